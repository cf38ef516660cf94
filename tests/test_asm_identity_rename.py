"""tools/asm_identity.py --per-kernel --rename: a function of REV is paired with its new name through the demangled names,
the pair is one row, and the function's own symbol does not count as a difference."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _s(symbol, body):
    """One function the way hipcc writes it: the Begin mark, the body, the descriptor lines that name the symbol."""
    return ["\t.globl\t%s ; -- Begin function %s\n" % (symbol, symbol), "%s:\n" % symbol, *("\t%s\n" % l for l in body),
            ".LBB3_1:\n", "\ts_endpgm\n", "\t.amdhsa_kernel %s\n" % symbol, "\t.set %s.num_vgpr, 4\n" % symbol]


def test_a_renamed_template_is_compared_as_one_row():
    import asm_identity as ai
    body = ["s_load_dword s0, s[0:1], 0x0", "v_mov_b32_e32 v0, s0"]
    old = _s("_Z6screenILi384ELb0EEvPj", body) + _s("_Z4bandPj", body) + _s("_Z4keptPj", body) + _s("_Z4gonePj", body)
    new = (_s("_Z6streamILi384ELb0E5CountEvT1_", body) + _s("_Z5band2I5CountEvT_", body[:1] + ["v_mov_b32_e32 v1, s0"])
           + _s("_Z4keptPj", body) + _s("_Z5freshPj", body))
    renames = [(r"screen<(.*)>", r"stream<\1, Count>"), ("band", "band2<Count>"), ("gone", "nowhere")]
    rows = {r[2]: r[3:] for r in ai.per_kernel(("f", []), old, new, renames)}
    assert rows["_Z6screenILi384ELb0EEvPj -> _Z6streamILi384ELb0E5CountEvT1_"][0].startswith("identical")
    verdict, diff = rows["_Z4bandPj -> _Z5band2I5CountEvT_"]
    assert verdict == "DIFFERS in 2 lines" and diff == ["-v_mov_b32_e32 v0, s0", "+v_mov_b32_e32 v1, s0"]
    assert rows["_Z4keptPj"][0].startswith("identical")
    assert rows["_Z4gonePj"][0] == "removed" and rows["_Z5freshPj"][0] == "added"   # (a rename without a counterpart pairs nothing)
    assert len(rows) == 5                                                          # no renamed function is listed twice


def test_without_renames_the_rows_are_what_they_were():
    import asm_identity as ai
    body = ["s_nop 0"]
    rows = {r[2]: r[3] for r in ai.per_kernel(("f", []), _s("_Z1aPj", body) + _s("_Z1bPj", body), _s("_Z1aPj", body) + _s("_Z1cPj", body))}
    assert rows == {"_Z1aPj": "identical (7 lines)", "_Z1bPj": "removed", "_Z1cPj": "added"}
