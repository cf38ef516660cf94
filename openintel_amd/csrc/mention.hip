// mention.hip -- oi_mention_summary: the social_summary sums of the documents that CONTAIN a query's terms, per time bucket or
// per key of the documents' group attribute.
//
// The lexical member of the aggregation family.  Its siblings (oi_volume.h) decide a document by sim(q, d) >= t_q over a stream
// of the corpus; this one decides it by m(q, d) >= need_q, where m is the number of the query's DISTINCT terms with a posting
// for d, and reads the postings of the BM25 index instead (bm25.hip / bm25_stream.hip state the layout: a term's run for doc
// block blk is postings[cell_start[t * n_win + 2 blk] .. cell_start[t * n_win + 2 blk + 2]), an entry is {u32 doc_in_block, f32
// impact}, doc_in_block < OI_BM25_BLOCK_DOCS, a (term, doc) pair appears once).  Clauses 1 and 2 (filter, cell), the cell and
// the fold are the family's: vo_bucket / vo_key (oi_volume.h), sm_add / sm_fold (oi_summary_cell.h).  Every sum is an integer
// sum, so the records do not depend on the grid or on the order of the atomics.
//
//   mn_plan_kernel    one wave per query, one raw term per lane: the distinct terms in first-occurrence order, |D_q|, need_q
//                     and a "counts nothing" flag (empty query, need_q > |D_q|, more than OI_MAX_MENTION_TERMS raw terms).
//   mn_match_kernel   persistent workgroups over the tasks (doc block, query).  The match counts of a task's 32768 documents are
//                     byte counters in LDS, four to a u32 word: a posting adds 1 << 8 (doc & 3) to word doc >> 2 (an LDS atomic;
//                     a count never exceeds 64, so no byte carries).  After a barrier the workgroup sweeps the words: a byte
//                     >= need_q is a match, and only a match loads its attributes and its signal record, passes the filter, finds
//                     its cell and is added (sm_add).  The sweep zeroes every word it found set, so the counters are zero
//                     again when the workgroup's next task begins.  A task with fewer non-empty runs than need_q (all of them
//                     empty included) is skipped from its cell_start words alone; a flagged query has no runs.
//                     With at most MN_LDS_CELLS cells per query (a day of hourly buckets) the matches of a task are summed in
//                     a copy of the query's cells in LDS first, and only its non-zero words leave as global atomics at the end
//                     of the task: a term of every document would otherwise send one global atomic per document to a handful of
//                     addresses.  The sums are integers either way.
//   mn_finish_kernel  sm_fold of every cell into the caller's records.
#include "oi_summary_cell.h"
#include "oi_volume.h"

#define MN_THREADS 256
#define MN_BLOCK OI_BM25_BLOCK_DOCS
#define MN_WORDS (MN_BLOCK / 4)   // 32 KB of byte counters
// the plan of a query: MN_PLAN_WORDS u32 -- [0, 64) the distinct terms, then |D_q|, need_q, the flag, one word of padding
#define MN_PLAN_WORDS 68
#define MN_PLAN_ND 64
#define MN_PLAN_NEED 65
#define MN_PLAN_FLAG 66
#define MN_LDS_CELLS 64           // cells per query up to which a task sums in LDS first (4 KB)

static_assert(OI_MAX_MENTION_TERMS == 64u, "one raw term per lane of the plan's wave; a byte counter holds a count of 64");

// ------------------------------------------------------------------ the plan
__global__ __launch_bounds__(64) void mn_plan_kernel(const uint32_t *__restrict__ q_terms, const uint32_t *__restrict__ q_offsets,
                                                     const uint32_t *__restrict__ min_match, uint32_t *__restrict__ plan) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    const uint32_t lo = q_offsets[q], hi = q_offsets[q + 1];
    // (device offsets were not seen by the host: a query of more than 64 raw terms, or with its end before its start, reads
    // no term at all)
    const bool too_many = hi < lo || hi - lo > OI_MAX_MENTION_TERMS;
    const uint32_t n = too_many ? 0u : hi - lo;
    const uint32_t t = lane < n ? q_terms[lo + lane] : 0u;
    bool keep = lane < n;
    for (uint32_t i = 0; i + 1 < n; ++i) { // (uniform) an earlier lane with the same term: a repeated term counts once
        const uint32_t ti = (uint32_t)__shfl((int)t, (int)i, OI_WAVE);
        if (i < lane && ti == t) keep = false;
    }
    const unsigned long long m = __ballot(keep);
    uint32_t *p = plan + (uint64_t)q * MN_PLAN_WORDS;
    if (keep) p[__popcll(m & ((1ull << lane) - 1ull))] = t;
    if (lane == 0) {
        const uint32_t nd = (uint32_t)__popcll(m);
        const uint32_t mm = min_match ? min_match[q] : 1u;
        const uint32_t need = (min_match && mm == 0u) ? nd : mm;
        p[MN_PLAN_ND] = nd;
        p[MN_PLAN_NEED] = need;
        p[MN_PLAN_FLAG] = (too_many || nd == 0u || need > nd) ? 1u : 0u;
    }
}

// ------------------------------------------------------------------ the match
struct MnArgs {
    const uint2 *postings;      // {doc_in_block, impact bits}, term-major
    uint64_t n_postings;
    const uint32_t *cell_start; // [vocab * n_win + 1]
    const uint32_t *plan;       // [nq][MN_PLAN_WORDS]
    const uint4 *filt;          // FILT: [nq]
    const uint2 *attrs;         // {group, stamp} per local row; null when no clause reads them
    const uint2 *sig;           // the signal records
    uint32_t *cells;            // [nq][n_cells][SM_CELL_WORDS]
    uint64_t n_docs;
    uint32_t n_win, vocab, n_blocks, nq;
    uint32_t origin, width, n_cells; // clause 2: TIME {stamp_origin, bucket_width, n_cells}, KEY {key_mask, its shift, n_cells}
#ifdef OI_ABLATION
    uint32_t ablate;                 // OI_MENTION_ABLATE: 1 = no tally (matches found, nothing added), 2 = no LDS adds (timings only)
#endif
};

template <bool KEY_AXIS, bool FILT>
__global__ __launch_bounds__(MN_THREADS) void mn_match_kernel(const MnArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t cnt[MN_WORDS];
    __shared__ uint32_t s_lo[2][64], s_hi[2][64]; // the runs of a task, by distinct term; two tasks: the next one's are fetched early
    __shared__ __attribute__((aligned(16))) uint32_t lcell[MN_LDS_CELLS * SM_CELL_WORDS]; // the task's cells, all zero between tasks

    const uint32_t tid = threadIdx.x, lane = tid & 63;
    for (uint32_t v = tid; v < MN_WORDS; v += MN_THREADS) cnt[v] = 0u;
    for (uint32_t v = tid; v < MN_LDS_CELLS * SM_CELL_WORDS; v += MN_THREADS) lcell[v] = 0u;
    const bool in_lds = a.n_cells <= MN_LDS_CELLS; // (uniform)

    // Task `task` is (block task / nq, query (task % nq + rot) % nq): block-major, so that the workgroups at work together read
    // the same documents' attributes and records and add to different queries' cells; rot = floor(block * nq / grid) is the
    // number of the round in which a workgroup takes the block (tasks are dealt out grid at a time), so a workgroup meets another
    // query in every round and the blocks of one heavy query go to different workgroups whatever nq and the grid have in common.
    auto decode = [&](uint32_t task, uint32_t *q, uint32_t *blk) {
        *blk = task / a.nq;
        *q = (task % a.nq + (uint32_t)(((uint64_t)*blk * a.nq) / gridDim.x)) % a.nq;
    };
    // The runs of a task.  Every bound is held inside the postings.
    auto load_bounds = [&](uint32_t task, uint32_t buf) {
        if (tid < 64) {
            uint32_t q, blk;
            decode(task, &q, &blk);
            const uint32_t *p = a.plan + (uint64_t)q * MN_PLAN_WORDS;
            uint32_t lo = 0, hi = 0;
            if (p[MN_PLAN_FLAG] == 0u && tid < p[MN_PLAN_ND]) {
                const uint32_t t = p[tid];
                if (t < a.vocab) { // (a term outside the vocabulary occurs in no document)
                    const uint32_t *c = a.cell_start + (uint64_t)t * a.n_win + 2u * blk;
                    const uint64_t l = c[0], h = c[2];
                    hi = (uint32_t)(h < a.n_postings ? h : a.n_postings);
                    lo = l < hi ? (uint32_t)l : hi;
                }
            }
            s_lo[buf][tid] = lo;
            s_hi[buf][tid] = hi;
        }
    };

    const uint32_t n_tasks = a.n_blocks * a.nq;
    uint32_t task = blockIdx.x, buf = 0;
    if (task < n_tasks) load_bounds(task, 0);
    for (; task < n_tasks; task += gridDim.x, buf ^= 1u) {
        __syncthreads(); // the task's runs are in LDS; the sweep of the task before it has left every counter zero
        uint32_t q, blk;
        decode(task, &q, &blk);
        const uint32_t lo_l = s_lo[buf][lane], hi_l = s_hi[buf][lane];
        unsigned long long live = __ballot(hi_l > lo_l);
        const uint32_t need = a.plan[(uint64_t)q * MN_PLAN_WORDS + MN_PLAN_NEED];
        if (task + gridDim.x < n_tasks) load_bounds(task + gridDim.x, buf ^ 1u);
        if ((uint32_t)__popcll(live) < need || live == 0ull) continue; // (uniform) no document can reach need_q

        // every posting of every non-empty run counts its document once
        while (live) {
            const uint32_t j = (uint32_t)__builtin_ctzll(live);
            live &= live - 1ull;
            const uint32_t lo = s_lo[buf][j], hi = s_hi[buf][j];
            for (uint32_t i = lo + tid; i < hi; i += MN_THREADS) {
                const uint32_t raw = a.postings[i].x, d = raw & (MN_BLOCK - 1u);
#ifdef OI_ABLATION
                if (a.ablate & 2u) { if (raw == 0xFFFFFFFFu) cnt[0] = raw; continue; } // (the load stays)
#endif
                atomicAdd(&cnt[d >> 2], 1u << (8u * (d & 3u)));
            }
        }
        __syncthreads();

        // the sweep: a word (four documents) per thread and step, so that a wave's matches lie in 2 KB of attributes and of
        // records; the loads of a word's matches are issued together, the clauses follow
        const uint64_t base = (uint64_t)blk * MN_BLOCK;
        const uint32_t in_block = (uint32_t)(a.n_docs - base < MN_BLOCK ? a.n_docs - base : MN_BLOCK);
        uint4 f = make_uint4(0u, 0u, 0u, 0u);
        if constexpr (FILT) f = a.filt[q];
        const uint64_t cell0 = (uint64_t)q * a.n_cells;
        const bool with_attrs = FILT || KEY_AXIS || a.width != 0u;
        for (uint32_t wi = tid; wi < (in_block + 3u) / 4u; wi += MN_THREADS) {
            const uint32_t w = cnt[wi];
            if (w == 0u) continue;
            cnt[wi] = 0u;
            bool hit[4];
            uint2 at[4], sg[4];
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                hit[b] = ((w >> (8u * b)) & 255u) >= need && 4u * wi + b < in_block;
                at[b] = sg[b] = make_uint2(0u, 0u);
                if (hit[b]) {
                    const uint64_t doc = base + 4u * wi + b;
                    if (with_attrs) at[b] = a.attrs[doc];
                    sg[b] = a.sig[doc];
                }
            }
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                if (!hit[b]) continue;
                if constexpr (FILT)
                    if (!oi_doc_passes(f, at[b])) continue;
                uint32_t c = 0;
                bool ok;
                if constexpr (KEY_AXIS) ok = vo_key(at[b].x, a.origin, a.width, a.n_cells, &c);
                else ok = vo_bucket(at[b].y, a.origin, a.width, a.n_cells, &c);
                if (!ok) continue;
#ifdef OI_ABLATION
                if (a.ablate & 1u) { if (sg[b].y == 0xFFFFFFFFu) a.cells[0] = sg[b].x; continue; } // (the loads stay)
#endif
                if (in_lds) sm_add(lcell, c, sg[b]);
                else sm_add(a.cells, cell0 + c, sg[b]);
            }
        }
        if (in_lds) {
            // the task's sums leave: every non-zero count, and the 64-bit sum through the thread of its low word
            __syncthreads();
            for (uint32_t v = tid; v < a.n_cells * SM_CELL_WORDS; v += MN_THREADS) {
                const uint32_t k = v % SM_CELL_WORDS;
                uint32_t *g = a.cells + (cell0 + v / SM_CELL_WORDS) * SM_CELL_WORDS;
                if (k < 12u) {
                    const uint32_t x = lcell[v];
                    if (x) { atomicAdd(g + k, x); lcell[v] = 0u; }
                } else if (k == SM_CELL_SUM) {
                    const unsigned long long x = *reinterpret_cast<const unsigned long long *>(lcell + v);
                    if (x) {
                        atomicAdd(reinterpret_cast<unsigned long long *>(g + SM_CELL_SUM), x);
                        lcell[v] = 0u;
                        lcell[v + 1] = 0u;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------ the finish
__global__ __launch_bounds__(256) void mn_finish_kernel(const uint32_t *__restrict__ cells, uint64_t n_cells,
                                                        oi_social_counters *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += (uint64_t)gridDim.x * blockDim.x)
        sm_fold(cells + i * SM_CELL_WORDS, out + i);
}

// ------------------------------------------------------------------ host
// Device terms / offsets / min_match / filters in, device records [n_queries][n_cells] out; asynchronous on the ctx stream.
// The argument and state checks are the entry point's (api.hip).
int oi_launch_mention_summary(oi_index *idx, const uint32_t *d_terms, const uint32_t *d_offsets, uint32_t B, const oi_mention_spec &sp,
                              const uint32_t *d_min_match, const uint4 *d_filt, oi_social_counters *d_out) {
    static_assert(sizeof(oi_social_counters) == 64, "one record per cell");
    static_assert(sizeof(uint32_t) * (MN_WORDS + 2 * 2 * 64 + MN_LDS_CELLS * SM_CELL_WORDS) <= 64 * 1024, "two workgroups per CU at the least");
    oi_ctx *ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    const bool key_axis = sp.axis == OI_MENTION_AXIS_KEY;
    const uint64_t n_cells = (uint64_t)B * sp.n_cells;
    DevBuf &cb = ctx->buf("mention_cells"), &pb = ctx->buf("mention_plan");
    OI_CHECK(cb.ensure(n_cells * SM_CELL_WORDS * 4));
    OI_CHECK(pb.ensure((size_t)B * MN_PLAN_WORDS * 4));
    OI_HIP_CHECK(hipMemsetAsync(cb.p, 0, n_cells * SM_CELL_WORDS * 4, st));
    {
        ProfScope ps(ctx, "mention_plan");
        hipLaunchKernelGGL(mn_plan_kernel, dim3(B), dim3(64), 0, st, d_terms, d_offsets, d_min_match, pb.as<uint32_t>());
        OI_HIP_CHECK(hipGetLastError());
    }
    const uint64_t n_tasks = (uint64_t)idx->n_blocks * B;
    if (n_tasks) {
        MnArgs a;
        a.postings = idx->postings.as<uint2>();
        a.n_postings = idx->n_postings;
        a.cell_start = idx->cell_start.as<uint32_t>();
        a.plan = pb.as<uint32_t>();
        a.filt = d_filt;
        a.attrs = (key_axis || d_filt || sp.bucket_width) ? idx->doc_attrs.as<uint2>() : nullptr;
        a.sig = idx->signals.as<uint2>();
        a.cells = cb.as<uint32_t>();
        a.n_docs = idx->n_docs;
        a.n_win = idx->n_win;
        a.vocab = idx->vocab;
        a.n_blocks = idx->n_blocks;
        a.nq = B;
        a.origin = sp.stamp_origin;
        a.width = key_axis ? (uint32_t)__builtin_ctz(sp.stamp_origin) : sp.bucket_width;
        a.n_cells = sp.n_cells;
#ifdef OI_ABLATION
        a.ablate = oi_ablation_env("OI_MENTION_ABLATE") ? (uint32_t)atoi(oi_ablation_env("OI_MENTION_ABLATE")) : 0u;
#endif
        const dim3 grid((uint32_t)std::min<uint64_t>(n_tasks, (uint64_t)ctx->num_cus * 4));
        ProfScope ps(ctx, "mention");
        if (key_axis) {
            if (d_filt) hipLaunchKernelGGL((mn_match_kernel<true, true>), grid, dim3(MN_THREADS), 0, st, a);
            else hipLaunchKernelGGL((mn_match_kernel<true, false>), grid, dim3(MN_THREADS), 0, st, a);
        } else {
            if (d_filt) hipLaunchKernelGGL((mn_match_kernel<false, true>), grid, dim3(MN_THREADS), 0, st, a);
            else hipLaunchKernelGGL((mn_match_kernel<false, false>), grid, dim3(MN_THREADS), 0, st, a);
        }
        OI_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(mn_finish_kernel, dim3((uint32_t)std::min<uint64_t>((n_cells + 255) / 256, 1024)), dim3(256), 0, st,
                       cb.as<uint32_t>(), n_cells, d_out);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}
