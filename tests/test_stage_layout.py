"""csrc/oi_stage_layout.h on its own: a stand-alone program that includes nothing of the library but that header, compiled with
g++ -fsanitize=address,undefined and run.  It checks the rules of the type (ascending offsets, every offset a multiple of the
granule, an absent part costs nothing, total() = the last offset + the last part's room, size_t arithmetic at 2^32 - 1 rows)
and that three carve-ups of the library give, byte for byte, the totals of the hand-written formulas they replaced -- the
formulas are written out below as the expectation."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openintel_amd", "csrc")

PROGRAM = r"""
#include "oi_stage_layout.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond);   \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static size_t up(size_t b, size_t g) { return (b + g - 1) & ~(g - 1); }
static size_t up256(size_t b) { return up(b, 256); }

// the rules, for one granule and one list of part sizes (the last one is not 0)
static int rules(size_t granule, const std::vector<size_t> &bytes) {
    StageLayout lay(granule);
    std::vector<size_t> at;
    size_t before = 0;
    for (size_t b : bytes) {
        at.push_back(lay.add(b));
        CHECK(at.back() % granule == 0);
        CHECK(at.back() == before);                         // a part starts where the parts before it end
        CHECK(lay.total() == at.back() + up(b, granule));   // total() = the last offset + the last part's room
        CHECK(b != 0 || lay.total() == before);             // an absent part adds nothing
        before = lay.total();
    }
    for (size_t i = 0; i + 1 < at.size(); ++i) {
        CHECK(at[i] <= at[i + 1]);                          // ascending
        CHECK(bytes[i] != 0 || at[i] == at[i + 1]);         // an absent part shares the next part's offset
        CHECK(bytes[i] == 0 || at[i] + bytes[i] <= at[i + 1]); // a part's room holds it
    }
    return 0;
}

int main() {
    for (size_t g : {size_t(16), size_t(256)}) {
        if (rules(g, {1, 0, 17, g, 0, 0, 3 * g + 1, 4})) return 1;
        if (rules(g, {0, 0, 5})) return 1;
        if (rules(g, {g, 2 * g})) return 1;                 // whole granules: total() = the last offset + the last size itself
    }
    {   // whole granules again, spelled out
        StageLayout lay(256);
        const size_t a = lay.add(512), b = lay.add(0), c = lay.add(768);
        CHECK(a == 0 && b == 512 && c == 512 && lay.total() == c + 768);
    }
    {   // 2^32 - 1 rows of 4 B: nothing is computed in 32 bits
        const size_t n = 0xFFFFFFFFull, lb = sizeof(uint32_t) * n;
        StageLayout lay(256);
        const size_t a = lay.add(lb), b = lay.add(lb), c = lay.add(12);
        CHECK(a == 0 && b == 0x400000000ull && c == 0x800000000ull && lay.total() == 0x800000100ull);
        CHECK(b >= lb && b - lb < 256);
    }
    {   // at<T>: the typed pointer of a part
        alignas(16) unsigned char buf[64] = {0};
        StageLayout lay(16);
        lay.add(3);
        const size_t p = lay.add(8);
        *StageLayout::at<uint32_t>(buf, p) = 0xA1B2C3D4u;
        CHECK(p == 16 && buf[16] + buf[17] + buf[18] + buf[19] == 0xA1 + 0xB2 + 0xC3 + 0xD4 && buf[15] == 0 && buf[20] == 0);
    }
    {   // oi_label_summary, OI_HOST, ranked: K = 3, top = 5, n_docs = 300 -- [labels | records | keys | counts | qualified]
        const size_t K = 3, top = 5, n = 300, per_c = top;
        const size_t lb = up256(4 * n), rb = 64 * K * per_c, kb = up256(4 * K * per_c), cb = up256(4 * K);
        const size_t want = lb + up256(rb) + kb + 2 * cb;
        StageLayout lay(256);
        const size_t labels = lay.add(4 * n), records = lay.add(64 * K * per_c), keys = lay.add(4 * K * per_c), counts = lay.add(4 * K),
                     qualified = lay.add(4 * K);
        CHECK(lay.total() == want && want == 3072);
        CHECK(labels == 0 && records == lb && keys == lb + up256(rb) && counts == lb + up256(rb) + kb && qualified == lb + up256(rb) + kb + cb);
    }
    {   // oi_narratives_fit, OI_HOST: K = 4, dim = 64, n_docs = 300, 24 buckets, a filter --
        // [labels | labels | sums | counts | centroids | centroids | filters | moved | records]
        const size_t K = 4, dim = 64, n = 300, nb = 24;
        const size_t lb = up256(4 * n), sb = up256(8 * K * dim), cb = up256(8 * K), vb = up256(4 * K * dim), fb = up256(16 * K);
        const size_t rbytes = 64 * K * nb, rb = up256(rbytes);
        const size_t want = 2 * lb + sb + cb + 2 * vb + fb + 256 + rb;
        StageLayout lay(256);
        const size_t lab0 = lay.add(4 * n), lab1 = lay.add(4 * n), sums = lay.add(8 * K * dim), counts = lay.add(8 * K), c0 = lay.add(4 * K * dim),
                     c1 = lay.add(4 * K * dim), filt = lay.add(16 * K), moved = lay.add(256), rec = lay.add(rbytes);
        CHECK(lay.total() == want && want == 13568);
        CHECK(lab0 == 0 && lab1 == lb && sums == 2 * lb && counts == 2 * lb + sb && c0 == 2 * lb + sb + cb && c1 == 2 * lb + sb + cb + vb);
        CHECK(filt == 2 * lb + sb + cb + 2 * vb && moved == filt + fb && rec == filt + fb + 256);
        StageLayout dev(256); // OI_DEVICE: no records part
        for (size_t b : {4 * n, 4 * n, 8 * K * dim, 8 * K, 4 * K * dim, 4 * K * dim, 16 * K, size_t(256), size_t(0)}) dev.add(b);
        CHECK(dev.total() == want - rb);
    }
    {   // the "exemplars" workspace: n = 300, K = 3, dim = 64, top = 10, a bf16 corpus --
        // [open words | cluster states (32 B) | histograms (256 bins) | keys | slots | rounded centroids]
        const size_t n = 300, K = 3, dim = 64, top = 10, cluster = 32, bins = 256;
        const size_t want = 256 + up256(cluster * K) + up256(4 * K * bins) + up256(4 * n) + up256(8 * K * top) + up256(4 * K * dim);
        StageLayout lay(256);
        const size_t open = lay.add(256), cl = lay.add(cluster * K), hist = lay.add(4 * K * bins), keys = lay.add(4 * n), slots = lay.add(8 * K * top),
                     rounded = lay.add(4 * K * dim);
        CHECK(lay.total() == want && want == 5888);
        CHECK(open == 0 && cl == 256 && hist == 256 + up256(cluster * K) && keys == hist + up256(4 * K * bins));   // (keys: where the preset memset ends)
        CHECK(slots == keys + up256(4 * n) && rounded == slots + up256(8 * K * top));
        StageLayout f32(256); // an f32 corpus: no rounded centroids
        for (size_t b : {size_t(256), cluster * K, 4 * K * bins, 4 * n, 8 * K * top, size_t(0)}) f32.add(b);
        CHECK(f32.total() == want - up256(4 * K * dim));
    }
    std::printf("stage layout ok\n");
    return 0;
}
"""


def test_the_layout_type_alone_under_the_host_sanitizers(tmp_path):
    src, exe = tmp_path / "stage_layout_check.cpp", tmp_path / "stage_layout_check"
    src.write_text(PROGRAM)
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "stage layout ok" in r.stdout, (r.stdout, r.stderr)


def test_the_header_includes_nothing_but_cstddef_and_cstdint():
    with open(os.path.join(CSRC, "oi_stage_layout.h")) as f:
        includes = [l.split()[1] for l in f if l.startswith("#include")]
    assert includes == ["<cstddef>", "<cstdint>"]
