// api.hip -- the extern "C" surface of libopenintel_hip.so (see include/openintel_hip.h).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <set>

#include "oi_internal.h"

// ---------------------------------------------------------------- errors
static thread_local char g_err[512] = "";

void oi_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// Hardware queues.  HIP spreads the streams of a process over GPU_MAX_HW_QUEUES hardware queues (default 4), and two streams
// that share a queue run one after the other whatever their events allow.  A two-lane pipeline (oi_pipeline_*, or a host that
// drives views of an index itself) has seven streams in play -- the caller's, two lanes, the fusing stream, a BM25 side stream
// each -- so with 4 queues some share, and the lanes' overlap is lost: 0.55 ms per batch at a 1.25M-row shard against 0.465
// with 8 queues, ten runs each, tools/r05_pipeline_probe.py.  The runtime reads the variable when it initialises, so it is set
// when this library is LOADED (never overriding the host's own choice); a host that initialises HIP before loading the library
// sets it itself (bench.py and tests/conftest.py do).  It changes scheduling only, never a result.
__attribute__((constructor)) static void oi_ask_for_more_hw_queues() { (void)setenv("GPU_MAX_HW_QUEUES", "8", /*overwrite=*/0); }

extern "C" const char *oi_last_error(void) { return g_err; }
extern "C" int oi_abi_version(void) { return OI_ABI_VERSION; }

// ---------------------------------------------------------------- per-(kernel, device) one-shots
int oi_dyn_lds(oi_ctx *ctx, const void *kernel, size_t bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;
    std::lock_guard<std::mutex> g(mu);
    const auto key = std::make_pair(kernel, ctx->device);
    if (done.count(key)) return OI_OK;
    OI_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done.insert(key);
    return OI_OK;
}

// ---------------------------------------------------------------- buffers
std::atomic<uint64_t> g_oi_ws_epoch{1};

int DevBuf::ensure(size_t bytes) {
    if (bytes <= cap && p) return OI_OK;
    if (borrowed) { oi_set_error("internal: a borrowed buffer cannot grow"); return OI_ERR_STATE; }
    g_oi_ws_epoch.fetch_add(1); // captured launch sequences that hold the old pointer are stale from here on
    if (p) {
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    size_t want = (bytes + 255) & ~(size_t)255;
    if (want == 0) want = 256;
    OI_HIP_CHECK(hipMalloc(&p, want));
    cap = want;
    return OI_OK;
}
void DevBuf::release() {
    if (p) g_oi_ws_epoch.fetch_add(1);
    if (p && !borrowed) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    borrowed = false;
}

int PinBuf::ensure(size_t bytes) {
    if (bytes <= cap) return OI_OK;
    release();
    const size_t want = (bytes + 4095) & ~(size_t)4095;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) == hipSuccess) {
        pinned = true;
    } else { // no page-locked memory to be had (a locked-memory limit): pageable staging -- the same calls, staged by the runtime
        (void)hipGetLastError();
        p = aligned_alloc(4096, want);
        pinned = false;
        if (!p) { oi_set_error("host staging buffer: out of memory (%zu bytes)", want); return OI_ERR_HIP; }
    }
    cap = want;
    return OI_OK;
}
void PinBuf::release() {
    if (p) {
        if (pinned) (void)hipHostFree(p);
        else free(p);
    }
    p = nullptr;
    cap = 0;
}

// ---------------------------------------------------------------- profiling hooks
void oi_ctx::prof_begin(const char *tag) {
    ProfSpan s;
    // (timing only: without the system-scope fence a default event performs when it completes -- each pair sits between two
    // kernels of the timed step)
    if (hipEventCreateWithFlags(&s.a, hipEventDisableSystemFence) != hipSuccess ||
        hipEventCreateWithFlags(&s.b, hipEventDisableSystemFence) != hipSuccess) return;
    (void)hipEventRecord(s.a, stream);
    prof[tag].push_back(s);
}
void oi_ctx::prof_end(const char *tag) {
    auto it = prof.find(tag);
    if (it == prof.end() || it->second.empty()) return;
    (void)hipEventRecord(it->second.back().b, stream);
}

extern "C" int oi_profile_reset(oi_ctx *ctx, int enable) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> g(ctx->mu);
    for (auto &kv : ctx->prof)
        for (auto &s : kv.second) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
    ctx->prof.clear();
    for (const char *runs : {"volume_runs", "summary_runs", "groups_runs", "share_runs"}) {
        // the fallback-run counters of oi_similar_volume / _summary / _groups / _share ("volume_exact", "summary_exact", "groups_exact",
        // "share_exact") start over with the spans
        auto vr = ctx->ws.find(runs);
        if (vr != ctx->ws.end() && vr->second.p) (void)hipMemsetAsync(vr->second.p, 0, 16, ctx->stream);
    }
    ctx->prof_enabled = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
    return OI_OK;
}

extern "C" int oi_profile_read(oi_ctx *ctx, const char *kernel_tag, double *total_ms_out, uint64_t *launches_out) {
    if (!ctx || !kernel_tag) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    double total = 0.0;
    uint64_t n = 0;
    if (strncmp(kernel_tag, "flagword", 8) == 0) { // diagnostics: raw words of the ctx state flag buffer
        uint32_t w[4] = {0, 0, 0, 0};
        DevBuf &st = ctx->buf("state_flag");
        if (st.p) OI_HIP_CHECK(hipMemcpy(w, st.p, 16, hipMemcpyDeviceToHost));
        if (total_ms_out) *total_ms_out = (double)w[(kernel_tag[8] - '0') & 3];
        if (launches_out) *launches_out = 0;
        return OI_OK;
    }
    if (strcmp(kernel_tag, "graph_replays") == 0 || strcmp(kernel_tag, "graph_captures") == 0) { // diagnostics of oi_set_graph_replay
        if (total_ms_out) *total_ms_out = 0.0;
        if (launches_out) *launches_out = kernel_tag[6] == 'r' ? ctx->graph_replays : ctx->graph_captures;
        return OI_OK;
    }
    if (strcmp(kernel_tag, "spec_state") == 0) { // diagnostics of the speculative screen thresholds: failed checks seen so far, searches that speculated
        oi_spec_take_failure(ctx);
        if (total_ms_out) *total_ms_out = (double)ctx->spec_failures;
        if (launches_out) *launches_out = ctx->spec_searches;
        return OI_OK;
    }
    if (strcmp(kernel_tag, "screen_gate") == 0) { // diagnostics: did the last screened search fall back to the exact kernel?
        uint32_t g = 0;                          // (0 no, nonzero yes; -1 when no search has used the screen)
        if (ctx->last_screen_gate) OI_HIP_CHECK(hipMemcpy(&g, ctx->last_screen_gate, 4, hipMemcpyDeviceToHost));
        if (total_ms_out) *total_ms_out = ctx->last_screen_gate ? (double)g : -1.0;
        if (launches_out) *launches_out = 0;
        return OI_OK;
    }
    if (strcmp(kernel_tag, "screen_width") == 0) { // diagnostics: workgroups of the last screened search's widest screen launch; the CUs
        if (total_ms_out) *total_ms_out = (double)ctx->last_screen_wgs;
        if (launches_out) *launches_out = (uint64_t)ctx->num_cus;
        return OI_OK;
    }
    if (strcmp(kernel_tag, "screen_sample") == 0) { // diagnostics: rows of the last search's sample pass (search.hip), 0 = it took none
        if (total_ms_out) *total_ms_out = (double)ctx->last_sample_rows;
        if (launches_out) *launches_out = 0;
        return OI_OK;
    }
    if (strcmp(kernel_tag, "rescreen_tier") == 0) { // diagnostics: the second tier of the last search's int8 route: 0 the bf16 rescreen,
        if (total_ms_out) *total_ms_out = (double)ctx->last_rescreen_tier; // 1 the residual plane's, -1 the search took another route
        if (launches_out) *launches_out = 0;
        return OI_OK;
    }
    if (strcmp(kernel_tag, "rescreen_survivors") == 0) { // diagnostics: keys the last int8-route search's second margin select kept,
        std::vector<uint32_t> c(ctx->last_rescreen_cnt ? ctx->last_rescreen_b : 0); // summed over the queries; the largest of one query
        if (!c.empty()) OI_HIP_CHECK(hipMemcpy(c.data(), ctx->last_rescreen_cnt, sizeof(uint32_t) * c.size(), hipMemcpyDeviceToHost));
        uint64_t sum = 0, mx = 0;
        for (uint32_t v : c) { sum += v; mx = std::max<uint64_t>(mx, v); }
        if (total_ms_out) *total_ms_out = (double)sum;
        if (launches_out) *launches_out = mx;
        return OI_OK;
    }
    if (strcmp(kernel_tag, "volume_state") == 0 || strcmp(kernel_tag, "summary_state") == 0 || strcmp(kernel_tag, "groups_state") == 0 ||
        strcmp(kernel_tag, "share_state") == 0) {
        // diagnostics of the last oi_similar_volume / oi_similar_summary / oi_similar_groups / oi_similar_share: undecided pairs its stream sent to the band (may exceed
        // the 4 Mi the buffer holds); bit 0 = a query had no bound, bit 1 = band overflow
        uint32_t w[4] = {0, 0, 0, 0};
        auto vs = ctx->ws.find(kernel_tag);
        if (vs != ctx->ws.end() && vs->second.p) OI_HIP_CHECK(hipMemcpy(w, vs->second.p, 16, hipMemcpyDeviceToHost));
        if (total_ms_out) *total_ms_out = (double)w[2];
        if (launches_out) *launches_out = (w[0] ? 1u : 0u) | (w[1] ? 2u : 0u);
        return OI_OK;
    }
    auto it = ctx->prof.find(kernel_tag);
    if (it != ctx->prof.end())
        for (auto &s : it->second) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { total += ms; ++n; }
        }
    const char *family = strcmp(kernel_tag, "volume_exact") == 0 ? "volume" : strcmp(kernel_tag, "summary_exact") == 0 ? "summary"
                       : strcmp(kernel_tag, "groups_exact") == 0 ? "groups" : strcmp(kernel_tag, "share_exact") == 0 ? "share" : nullptr;
    if (family) {
        // the gated fallback inside screened oi_similar_volume / _summary / _groups / _share calls ("volume_fallback", "summary_fallback",
        // "groups_fallback", "share_fallback": launched every time, exits at once unless the call needs it) counts here only for the runs that really
        // counted a batch (cosine_volume.hip, cosine_summary.hip, cosine_groups.hip)
        uint32_t runs = 0;
        auto vr = ctx->ws.find(std::string(family) + "_runs");
        if (vr != ctx->ws.end() && vr->second.p) OI_HIP_CHECK(hipMemcpy(&runs, vr->second.p, 4, hipMemcpyDeviceToHost));
        auto fb = ctx->prof.find(std::string(family) + "_fallback");
        if (runs && fb != ctx->prof.end()) {
            for (auto &s : fb->second) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) total += ms;
            }
            n += runs;
        }
    }
    if (total_ms_out) *total_ms_out = total;
    if (launches_out) *launches_out = n;
    return OI_OK;
}

// ---------------------------------------------------------------- captured launch sequences (hipGraph replay)
#define OI_MAX_GRAPHS 32

// (callers make sure no launch of the graph is still in flight: every path that frees one synchronises the ctx stream first)
static void graph_free(GraphEntry &e) {
    if (e.exec) (void)hipGraphExecDestroy(e.exec);
    if (e.graph) (void)hipGraphDestroy(e.graph);
    e.exec = nullptr;
    e.graph = nullptr;
}

static void graphs_purge(oi_ctx *ctx, uint64_t index_uid) { // index_uid 0 = all
    for (size_t i = 0; i < ctx->graphs.size();)
        if (index_uid == 0 || ctx->graphs[i].key[0] == index_uid) {
            graph_free(ctx->graphs[i]);
            ctx->graphs.erase(ctx->graphs.begin() + (long)i);
        } else ++i;
}

// body(): the launches of one call, all on ctx->stream (and streams forked from and joined back into it), nothing that
// synchronises.  First call with a key: eager (it also allocates the workspaces and sets the kernels' attributes);
// second: captured, instantiated, launched; afterwards: one hipGraphLaunch.  Anything unusual -- profiling on, the default
// stream, a workspace that moved, a capture that fails -- takes the eager path, which is always correct.
template <class F> static int run_captured(oi_ctx *ctx, const uint64_t (&key)[10], F &&body) {
    if (!ctx->use_graphs || ctx->prof_enabled || !ctx->stream) return body();
    const uint64_t epoch = g_oi_ws_epoch.load();
    GraphEntry *e = nullptr;
    for (auto &g : ctx->graphs)
        if (memcmp(g.key, key, sizeof(key)) == 0) { e = &g; break; }
    if (!e) {
        if (ctx->graphs.size() >= OI_MAX_GRAPHS) {
            size_t lru = 0;
            for (size_t i = 1; i < ctx->graphs.size(); ++i)
                if (ctx->graphs[i].last_use < ctx->graphs[lru].last_use) lru = i;
            OI_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // rare (more than OI_MAX_GRAPHS distinct calls): its last replay may still run
            graph_free(ctx->graphs[lru]);
            ctx->graphs.erase(ctx->graphs.begin() + (long)lru);
        }
        ctx->graphs.emplace_back();
        e = &ctx->graphs.back();
        memcpy(e->key, key, sizeof(key));
        e->last_use = ++ctx->graph_clock;
        const int rc = body();
        e->epoch = g_oi_ws_epoch.load(); // (after the call: whatever it allocated is in place now)
        return rc;
    }
    e->last_use = ++ctx->graph_clock;
    if (e->epoch != epoch) { // a workspace moved since: start over (eager now, capture next time)
        OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        graph_free(*e);
        e->state = 0;
        const int rc = body();
        e->epoch = g_oi_ws_epoch.load();
        return rc;
    }
    if (e->state == 2) return body();
    if (e->state == 1) {
        OI_HIP_CHECK(hipGraphLaunch(e->exec, ctx->stream));
        ++ctx->graph_replays;
        return OI_OK;
    }
    // state 0, same epoch: capture
    if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed) != hipSuccess) {
        (void)hipGetLastError();
        e->state = 2;
        return body();
    }
    const int rc = body();
    hipGraph_t g = nullptr;
    const hipError_t end = hipStreamEndCapture(ctx->stream, &g);
    if (rc != OI_OK || end != hipSuccess || !g || g_oi_ws_epoch.load() != epoch) {
        (void)hipGetLastError();
        if (g) (void)hipGraphDestroy(g);
        e->state = 2;
        if (rc != OI_OK) return rc; // (nothing of the failed call was launched)
        return body();               // the captured launches never ran: run them
    }
    hipGraphExec_t x = nullptr;
    if (hipGraphInstantiate(&x, g, nullptr, nullptr, 0) != hipSuccess || !x) {
        (void)hipGetLastError();
        (void)hipGraphDestroy(g);
        e->state = 2;
        return body();
    }
    e->graph = g;
    e->exec = x;
    e->state = 1;
    ++ctx->graph_captures;
    OI_HIP_CHECK(hipGraphLaunch(e->exec, ctx->stream));
    return OI_OK;
}

extern "C" int oi_set_graph_replay(oi_ctx *ctx, int enable) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->use_graphs = enable != 0;
    if (!ctx->use_graphs) {
        OI_HIP_CHECK(hipSetDevice(ctx->device));
        OI_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // no replay in flight when its graph goes
        graphs_purge(ctx, 0);
    }
    return OI_OK;
}

// ---------------------------------------------------------------- ctx
extern "C" int oi_create(int device_ordinal, oi_ctx **out) {
    if (!out) { oi_set_error("oi_create: out is null"); return OI_ERR_INVALID_ARG; }
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        oi_set_error("oi_create: no HIP device visible (this library has no CPU fallback)");
        return OI_ERR_NO_DEVICE;
    }
    OI_REQUIRE(device_ordinal >= 0 && device_ordinal < n, "oi_create: device %d of %d", device_ordinal, n);
    OI_HIP_CHECK(hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    OI_HIP_CHECK(hipGetDeviceProperties(&prop, device_ordinal));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        oi_set_error("oi_create: device %d is %s; this library is built for gfx950 only", device_ordinal,
                     prop.gcnArchName);
        return OI_ERR_NO_DEVICE;
    }
    oi_ctx *c = new oi_ctx();
    c->device = device_ordinal;
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->stream = nullptr;
    if (const char *m = getenv("OI_COSINE_MODE"))
        c->cosine_mode = strcmp(m, "split") == 0 ? OI_COSINE_SPLIT : strcmp(m, "exact") == 0 ? OI_COSINE_EXACT
                         : strcmp(m, "screen-copy") == 0 ? OI_COSINE_SCREEN_COPY
                         : strcmp(m, "screen-stream") == 0 ? OI_COSINE_SCREEN_STREAM : OI_COSINE_SCREEN;
    // best effort: without these the two legs of a query simply run one after the other.  The side stream itself is made by
    // the first hybrid search of the context (ensure_side_stream): a context that never runs one -- the fusing context of a
    // pipeline, a lexicon-only host -- does not take one of the process's few hardware queues (HIP hands streams of one priority
    // out over GPU_MAX_HW_QUEUES = 4 of them; two streams on one queue run one after the other whatever the events say).
    // (fork / join ORDER the side stream's kernels against the main stream's through hipStreamWaitEvent: they keep the default
    // fence -- hipEventDisableSystemFence is documented for timing events only; the ~12 us it saved per step in round 4 rested
    // on the kernels' own release semantics, an implementation detail of the runtime)
    if (hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess) c->ev_fork = nullptr;
    if (hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) c->ev_join = nullptr;
    *out = c;
    return OI_OK;
}

extern "C" int oi_create_like(oi_ctx *like, oi_ctx **out) {
    if (!out) { oi_set_error("oi_create_like: out is null"); return OI_ERR_INVALID_ARG; }
    *out = nullptr;
    if (!like) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    OI_CHECK(oi_create(like->device, out));
    std::lock_guard<std::mutex> g(like->mu);
    (*out)->cosine_mode = like->cosine_mode;
    (*out)->overlap_legs = like->overlap_legs;
    (*out)->speculate = like->speculate;
    (*out)->rescreen_residual = like->rescreen_residual;
    (*out)->use_graphs = like->use_graphs;
    return OI_OK;
}

// The teardown proper: runs when the last reference goes (the caller's handle, or the last index that outlived it).
static void ctx_release(oi_ctx *ctx) {
    if (ctx->refs.fetch_sub(1) != 1) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->side_stream) { (void)hipStreamSynchronize(ctx->side_stream); (void)hipStreamDestroy(ctx->side_stream); }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    oi_profile_reset(ctx, 0);
    graphs_purge(ctx, 0);
    for (auto &kv : ctx->ws) kv.second.release();
    ctx->pin_in.release();
    ctx->pin_out.release();
    if (ctx->spec_fail_host) (void)hipHostFree(ctx->spec_fail_host);
    delete ctx;
}

extern "C" void oi_destroy(oi_ctx *ctx) {
    if (!ctx) return;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        // With indexes still alive the object stays (they search, and are destroyed, through it): from here on it runs
        // on the default stream -- the caller's stream may not outlive the caller's handle.
        if (ctx->refs.load() > 1) ctx->stream = nullptr;
    }
    ctx_release(ctx);
}

extern "C" int oi_workspace_bytes(oi_ctx *ctx, uint64_t *device_bytes, uint64_t *pinned_bytes) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> g(ctx->mu);
    uint64_t d = 0;
    for (auto &kv : ctx->ws)
        if (!kv.second.borrowed) d += kv.second.cap;
    if (device_bytes) *device_bytes = d;
    if (pinned_bytes) *pinned_bytes = (ctx->pin_in.pinned ? ctx->pin_in.cap : 0) + (ctx->pin_out.pinned ? ctx->pin_out.cap : 0);
    return OI_OK;
}

extern "C" int oi_set_stream(oi_ctx *ctx, void *hip_stream) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return OI_OK;
}

extern "C" int oi_set_cosine_mode(oi_ctx *ctx, int mode) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(mode == OI_COSINE_EXACT || mode == OI_COSINE_SPLIT || mode == OI_COSINE_SCREEN || mode == OI_COSINE_SCREEN_COPY ||
                   mode == OI_COSINE_SCREEN_STREAM,
               "oi_set_cosine_mode: unknown mode %d", mode);
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->cosine_mode = mode;
    return OI_OK;
}

extern "C" int oi_set_overlap(oi_ctx *ctx, int enable) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->overlap_legs = enable != 0;
    return OI_OK;
}

extern "C" int oi_set_screen_speculation(oi_ctx *ctx, int enable) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->speculate = enable != 0;
    ctx->spec_skip = ctx->spec_backoff = 0;
    return OI_OK;
}

// Not part of the C ABI (no declaration in include/openintel_hip.h): the second tier of the int8 route.  tier 1 (default): the
// residual plane's rescreen where the index holds the plane; tier 0: the bf16 rescreen whatever the index holds -- A/B runs and the
// tests take both tails over one index in one process.  The lists do not depend on it.
extern "C" int oi_internal_set_rescreen_tier(oi_ctx *ctx, int tier) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(tier == 0 || tier == 1, "oi_internal_set_rescreen_tier: unknown tier %d", tier);
    std::lock_guard<std::mutex> g(ctx->mu);
    g_oi_ws_epoch.fetch_add(1); // (captured query calls hold the other tail's launches)
    ctx->rescreen_residual = tier == 1;
    return OI_OK;
}

static int check_overflow_locked(oi_ctx *ctx) {
    DevBuf &st = ctx->buf("state_flag");
    if (!st.p) return OI_OK;
    uint32_t f = 0;
    OI_HIP_CHECK(hipMemcpyAsync(&f, st.p, sizeof(f), hipMemcpyDeviceToHost, ctx->stream));
    OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (f) {
        OI_HIP_CHECK(hipMemsetAsync(st.p, 0, 16, ctx->stream));
        oi_set_error("internal candidate pool overflowed");
        return OI_ERR_OVERFLOW;
    }
    return OI_OK;
}

extern "C" int oi_synchronize(oi_ctx *ctx) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return check_overflow_locked(ctx);
}

// ---------------------------------------------------------------- PostAnalyzer path
extern "C" int oi_lexicon_analyze_device(oi_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets,
                                         uint64_t n, uint64_t blob_bytes, double *d_pol, uint8_t *d_spec) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    if (n == 0) return OI_OK;
    OI_REQUIRE(d_offsets && d_pol && d_spec && (d_blob || blob_bytes == 0), "lexicon: null buffer");
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    return oi_launch_lexicon(ctx, d_blob, d_offsets, n, blob_bytes, d_pol, d_spec);
}

extern "C" int oi_lexicon_summary_device(oi_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets, uint64_t n,
                                         uint64_t blob_bytes, const uint8_t *d_sources, double tau, double *d_pol,
                                         uint8_t *d_spec, oi_social_counters *out) {
    if (!ctx || !out) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    if (n == 0) { memset(out, 0, sizeof(*out)); return OI_OK; }
    OI_REQUIRE(d_offsets && (d_blob || blob_bytes == 0), "lexicon summary: null buffer");
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    return oi_launch_lexicon_fused(ctx, d_blob, d_offsets, n, blob_bytes, d_pol, d_spec, d_sources, tau, out);
}

extern "C" int oi_lexicon_analyze(oi_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, uint64_t n,
                                  double *pol_out, uint8_t *spec_out) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    if (n == 0) return OI_OK;
    OI_REQUIRE(offsets && pol_out && spec_out, "lexicon: null buffer");
    OI_REQUIRE(offsets[0] == 0, "lexicon: offsets[0] must be 0");
    const uint64_t bytes = offsets[n];
    OI_REQUIRE(blob || bytes == 0, "lexicon: null text blob");
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // A ticker's posts (the reference's call: <= 100 posts, ~20 KB) are a launch-latency call: text and offsets go through
    // the context's page-locked buffer in ONE DMA, the signals come back in one (100 posts: 62 -> 41 us per call, 10 posts: 49 -> 29; tools/analyze_latency_probe.py).
    const size_t off_o = (bytes + 15) & ~(size_t)15, in_bytes = off_o + sizeof(uint64_t) * (n + 1);
    const size_t out_bytes = sizeof(double) * n + n;
    if (in_bytes <= OI_PINNED_STAGE_MAX) {
        DevBuf &si = ctx->buf("lex_stage_in"), &so = ctx->buf("lex_stage_out");
        OI_CHECK(si.ensure(in_bytes + 64));
        OI_CHECK(so.ensure(out_bytes));
        OI_CHECK(ctx->pin_in.ensure(in_bytes));
        OI_CHECK(ctx->pin_out.ensure(out_bytes));
        uint8_t *h = ctx->pin_in.as<uint8_t>();
        if (bytes) memcpy(h, blob, bytes);
        memcpy(h + off_o, offsets, sizeof(uint64_t) * (n + 1));
        OI_HIP_CHECK(hipMemcpyAsync(si.p, h, in_bytes, hipMemcpyHostToDevice, st));
        double *d_pol = so.as<double>();
        uint8_t *d_spec = so.as<uint8_t>() + sizeof(double) * n;
        OI_CHECK(oi_launch_lexicon(ctx, si.as<uint8_t>(), reinterpret_cast<const uint64_t *>(si.as<uint8_t>() + off_o), n, bytes,
                                   d_pol, d_spec));
        OI_HIP_CHECK(hipMemcpyAsync(ctx->pin_out.p, so.p, out_bytes, hipMemcpyDeviceToHost, st));
        OI_HIP_CHECK(hipStreamSynchronize(st));
        memcpy(pol_out, ctx->pin_out.p, sizeof(double) * n);
        memcpy(spec_out, ctx->pin_out.as<uint8_t>() + sizeof(double) * n, n);
        return OI_OK;
    }
    DevBuf &b = ctx->buf("lex_blob"), &o = ctx->buf("lex_off"), &p = ctx->buf("lex_pol"), &s = ctx->buf("lex_spec");
    OI_CHECK(b.ensure(bytes + 64));
    OI_CHECK(o.ensure(sizeof(uint64_t) * (n + 1)));
    OI_CHECK(p.ensure(sizeof(double) * n));
    OI_CHECK(s.ensure(n));
    if (bytes) OI_HIP_CHECK(hipMemcpyAsync(b.p, blob, bytes, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemcpyAsync(o.p, offsets, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, st));
    OI_CHECK(oi_launch_lexicon(ctx, b.as<uint8_t>(), o.as<uint64_t>(), n, bytes, p.as<double>(), s.as<uint8_t>()));
    OI_HIP_CHECK(hipMemcpyAsync(pol_out, p.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipMemcpyAsync(spec_out, s.p, n, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipStreamSynchronize(st));
    return OI_OK;
}

extern "C" int oi_headline_scan_device(oi_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets, uint64_t n,
                                       uint64_t blob_bytes, const uint8_t *ticker, uint64_t ticker_len,
                                       const uint8_t *forms_blob, const uint32_t *form_offsets, uint32_t n_forms,
                                       uint16_t *d_mask, uint64_t *d_order, uint8_t *d_about) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    if (n == 0) return OI_OK;
    OI_REQUIRE(d_offsets && d_mask && d_order && d_about && (d_blob || blob_bytes == 0), "headline scan: null buffer");
    OI_REQUIRE((ticker || ticker_len == 0) && (n_forms == 0 || (forms_blob && form_offsets)),
               "headline scan: null ticker/forms");
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    return oi_launch_headline_scan(ctx, d_blob, d_offsets, n, blob_bytes, ticker, ticker_len, forms_blob,
                                   form_offsets, n_forms, d_mask, d_order, d_about);
}

extern "C" int oi_headline_scan(oi_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, uint64_t n,
                                const uint8_t *ticker, uint64_t ticker_len, const uint8_t *forms_blob,
                                const uint32_t *form_offsets, uint32_t n_forms, uint16_t *mask_out,
                                uint64_t *order_out, uint8_t *about_out) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    if (n == 0) return OI_OK;
    OI_REQUIRE(offsets && mask_out && order_out && about_out, "headline scan: null buffer");
    OI_REQUIRE(offsets[0] == 0, "headline scan: offsets[0] must be 0");
    OI_REQUIRE((ticker || ticker_len == 0) && (n_forms == 0 || (forms_blob && form_offsets)),
               "headline scan: null ticker/forms");
    const uint64_t bytes = offsets[n];
    OI_REQUIRE(blob || bytes == 0, "headline scan: null title blob");
    for (uint64_t i = 0; i < n; ++i)
        OI_REQUIRE(offsets[i + 1] >= offsets[i] && offsets[i + 1] - offsets[i] < (1ull << 32),
                   "headline scan: offsets must ascend and a title must be shorter than 4 GiB");
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the dip gate's own call is a handful of headlines per ticker (dip.rs:617-626): like oi_lexicon_analyze, a small call
    // goes through the page-locked buffers -- titles + offsets in one DMA, order | mask | about back in one
    const size_t off_o = (bytes + 15) & ~(size_t)15, in_bytes = off_o + sizeof(uint64_t) * (n + 1);
    const size_t out_m = sizeof(uint64_t) * n, out_a = out_m + sizeof(uint16_t) * n, out_bytes = out_a + n;
    if (in_bytes <= OI_PINNED_STAGE_MAX) {
        DevBuf &si = ctx->buf("hl_stage_in"), &so = ctx->buf("hl_stage_out");
        OI_CHECK(si.ensure(in_bytes + 64));
        OI_CHECK(so.ensure(out_bytes));
        OI_CHECK(ctx->pin_in.ensure(in_bytes));
        OI_CHECK(ctx->pin_out.ensure(out_bytes));
        uint8_t *h = ctx->pin_in.as<uint8_t>();
        if (bytes) memcpy(h, blob, bytes);
        memcpy(h + off_o, offsets, sizeof(uint64_t) * (n + 1));
        OI_HIP_CHECK(hipMemcpyAsync(si.p, h, in_bytes, hipMemcpyHostToDevice, st));
        uint8_t *d = so.as<uint8_t>();
        OI_CHECK(oi_launch_headline_scan(ctx, si.as<uint8_t>(), reinterpret_cast<const uint64_t *>(si.as<uint8_t>() + off_o), n,
                                         bytes, ticker, ticker_len, forms_blob, form_offsets, n_forms,
                                         reinterpret_cast<uint16_t *>(d + out_m), reinterpret_cast<uint64_t *>(d), d + out_a));
        OI_HIP_CHECK(hipMemcpyAsync(ctx->pin_out.p, so.p, out_bytes, hipMemcpyDeviceToHost, st));
        OI_HIP_CHECK(hipStreamSynchronize(st));
        const uint8_t *r = ctx->pin_out.as<uint8_t>();
        memcpy(order_out, r, out_m);
        memcpy(mask_out, r + out_m, sizeof(uint16_t) * n);
        memcpy(about_out, r + out_a, n);
        return OI_OK;
    }
    DevBuf &b = ctx->buf("hl_blob"), &o = ctx->buf("hl_off"), &m = ctx->buf("hl_mask"), &r = ctx->buf("hl_order"),
           &a = ctx->buf("hl_about");
    OI_CHECK(b.ensure(bytes + 64));
    OI_CHECK(o.ensure(sizeof(uint64_t) * (n + 1)));
    OI_CHECK(m.ensure(sizeof(uint16_t) * n));
    OI_CHECK(r.ensure(sizeof(uint64_t) * n));
    OI_CHECK(a.ensure(n));
    if (bytes) OI_HIP_CHECK(hipMemcpyAsync(b.p, blob, bytes, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemcpyAsync(o.p, offsets, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, st));
    OI_CHECK(oi_launch_headline_scan(ctx, b.as<uint8_t>(), o.as<uint64_t>(), n, bytes, ticker, ticker_len, forms_blob,
                                     form_offsets, n_forms, m.as<uint16_t>(), r.as<uint64_t>(), a.as<uint8_t>()));
    OI_HIP_CHECK(hipMemcpyAsync(mask_out, m.p, sizeof(uint16_t) * n, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipMemcpyAsync(order_out, r.p, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipMemcpyAsync(about_out, a.p, n, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipStreamSynchronize(st));
    return OI_OK;
}

// The dip screen's headline gate over the ROWS of a scan (application/dip.rs: one `check` per loser, each calling the gate
// of domain/dip.rs:612-659 on its own headlines with its own ticker and name forms): one staging copy of all titles, one
// launch per row back to back on the stream, one copy back, one synchronise.
extern "C" int oi_headline_scan_rows(oi_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, uint64_t n,
                                     const uint64_t *row_offsets, uint32_t n_rows, const uint8_t *tickers_blob,
                                     const uint32_t *ticker_offsets, const uint8_t *forms_blob, const uint32_t *form_offsets,
                                     const uint32_t *row_form_offsets, uint16_t *mask_out, uint64_t *order_out,
                                     uint8_t *about_out) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    if (n_rows == 0) return OI_OK;
    OI_REQUIRE(n_rows <= 4096, "headline rows: at most 4096 rows per call (%u given)", n_rows);
    OI_REQUIRE(row_offsets && ticker_offsets && row_form_offsets, "headline rows: null row table");
    OI_REQUIRE(row_offsets[0] == 0 && row_offsets[n_rows] == n, "headline rows: the rows must cover titles [0, %llu)",
               (unsigned long long)n);
    for (uint32_t r = 0; r < n_rows; ++r)
        OI_REQUIRE(row_offsets[r] <= row_offsets[r + 1] && ticker_offsets[r] <= ticker_offsets[r + 1] &&
                       row_form_offsets[r] <= row_form_offsets[r + 1],
                   "headline rows: row %u has descending offsets", r);
    OI_REQUIRE(tickers_blob || ticker_offsets[n_rows] == 0, "headline rows: null tickers");
    OI_REQUIRE(row_form_offsets[n_rows] == 0 || (forms_blob && form_offsets), "headline rows: null forms");
    if (n == 0) return OI_OK;
    OI_REQUIRE(offsets && mask_out && order_out && about_out, "headline rows: null buffer");
    OI_REQUIRE(offsets[0] == 0, "headline rows: offsets[0] must be 0");
    const uint64_t bytes = offsets[n];
    OI_REQUIRE(blob || bytes == 0, "headline rows: null title blob");
    for (uint64_t i = 0; i < n; ++i)
        OI_REQUIRE(offsets[i + 1] >= offsets[i] && offsets[i + 1] - offsets[i] < (1ull << 32),
                   "headline rows: offsets must ascend and a title must be shorter than 4 GiB");
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // staging: [titles | offsets | one table set per row] in, [order | mask | about] out
    const size_t pb = oi_headline_params_bytes();
    const size_t off_o = (bytes + 15) & ~(size_t)15, off_p = (off_o + sizeof(uint64_t) * (n + 1) + 15) & ~(size_t)15;
    const size_t in_bytes = off_p + pb * n_rows;
    const size_t out_m = sizeof(uint64_t) * n, out_a = out_m + sizeof(uint16_t) * n, out_bytes = out_a + n;
    DevBuf &si = ctx->buf("hl_rows_in"), &so = ctx->buf("hl_rows_out");
    OI_CHECK(si.ensure(in_bytes + 64));
    OI_CHECK(so.ensure(out_bytes));
    // page-locked staging for the calls it pays for (one ticker's or a dip scan's rows); a large scan packs into pageable
    // memory and copies its results straight into the caller's arrays -- PinBuf never shrinks, and one big call would leave
    // tens of MB page-locked for the life of the ctx (the other OI_HOST entry points follow the same rule)
    const bool pin = in_bytes <= OI_PINNED_STAGE_MAX && out_bytes <= OI_PINNED_STAGE_MAX;
    std::vector<uint8_t> pageable_in;
    uint8_t *h;
    if (pin) {
        OI_CHECK(ctx->pin_in.ensure(in_bytes));
        OI_CHECK(ctx->pin_out.ensure(out_bytes));
        h = ctx->pin_in.as<uint8_t>();
    } else {
        pageable_in.resize(in_bytes);
        h = pageable_in.data();
    }
    if (bytes) memcpy(h, blob, bytes);
    memcpy(h + off_o, offsets, sizeof(uint64_t) * (n + 1));
    for (uint32_t r = 0; r < n_rows; ++r)
        OI_CHECK(oi_headline_build_params(h + off_p + pb * r, tickers_blob ? tickers_blob + ticker_offsets[r] : nullptr,
                                          ticker_offsets[r + 1] - ticker_offsets[r], forms_blob,
                                          form_offsets ? form_offsets + row_form_offsets[r] : nullptr,
                                          row_form_offsets[r + 1] - row_form_offsets[r]));
    OI_HIP_CHECK(hipMemcpyAsync(si.p, h, in_bytes, hipMemcpyHostToDevice, st));
    uint8_t *d = si.as<uint8_t>(), *o = so.as<uint8_t>();
    const uint64_t *d_offs = reinterpret_cast<const uint64_t *>(d + off_o);
    for (uint32_t r = 0; r < n_rows; ++r) {
        const uint64_t t0 = row_offsets[r], t1 = row_offsets[r + 1];
        if (t1 == t0) continue;
        OI_CHECK(oi_launch_headline_scan_params(ctx, d, d_offs + t0, t1 - t0, bytes, offsets[t1] - offsets[t0], d + off_p + pb * r,
                                                reinterpret_cast<uint16_t *>(o + out_m) + t0,
                                                reinterpret_cast<uint64_t *>(o) + t0, o + out_a + t0));
    }
    if (!pin) {
        OI_HIP_CHECK(hipMemcpyAsync(order_out, o, out_m, hipMemcpyDeviceToHost, st));
        OI_HIP_CHECK(hipMemcpyAsync(mask_out, o + out_m, sizeof(uint16_t) * n, hipMemcpyDeviceToHost, st));
        OI_HIP_CHECK(hipMemcpyAsync(about_out, o + out_a, n, hipMemcpyDeviceToHost, st));
        OI_HIP_CHECK(hipStreamSynchronize(st)); // (before pageable_in goes out of scope)
        return OI_OK;
    }
    OI_HIP_CHECK(hipMemcpyAsync(ctx->pin_out.p, so.p, out_bytes, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipStreamSynchronize(st));
    const uint8_t *rr = ctx->pin_out.as<uint8_t>();
    memcpy(order_out, rr, out_m);
    memcpy(mask_out, rr + out_m, sizeof(uint16_t) * n);
    memcpy(about_out, rr + out_a, n);
    return OI_OK;
}

extern "C" int oi_social_summary(oi_ctx *ctx, const uint8_t *sources, uint64_t n_posts, const double *polarity,
                                 const uint8_t *speculative, uint64_t n_signals, double tau, int location,
                                 oi_social_counters *out) {
    if (!ctx || !out) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    if (n_signals != n_posts) { // speculation_engine.rs:29-34
        oi_set_error("analyzer returned %llu signals for %llu posts", (unsigned long long)n_signals,
                     (unsigned long long)n_posts);
        return OI_ERR_ANALYZER_MISMATCH;
    }
    const uint64_t n = n_posts;
    if (n == 0) { memset(out, 0, sizeof(*out)); return OI_OK; }
    OI_REQUIRE(polarity && speculative, "social_summary: null buffer");
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    if (location == OI_DEVICE) return oi_launch_social_summary(ctx, sources, polarity, speculative, n, tau, out);
    hipStream_t st = ctx->stream;
    DevBuf &s = ctx->buf("sum_src"), &p = ctx->buf("sum_pol"), &f = ctx->buf("sum_spec");
    OI_CHECK(p.ensure(sizeof(double) * n));
    OI_CHECK(f.ensure(n));
    OI_HIP_CHECK(hipMemcpyAsync(p.p, polarity, sizeof(double) * n, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemcpyAsync(f.p, speculative, n, hipMemcpyHostToDevice, st));
    const uint8_t *dsrc = nullptr;
    if (sources) {
        OI_CHECK(s.ensure(n));
        OI_HIP_CHECK(hipMemcpyAsync(s.p, sources, n, hipMemcpyHostToDevice, st));
        dsrc = s.as<uint8_t>();
    }
    return oi_launch_social_summary(ctx, dsrc, p.as<double>(), f.as<uint8_t>(), n, tau, out);
}

// Per-segment sums of a pooled batch (the batch callers: mcp/tools.rs:193-225, :303-352).
extern "C" int oi_social_summary_segmented(oi_ctx *ctx, const uint8_t *sources, const double *polarity,
                                           const uint8_t *speculative, uint64_t n_posts, const uint64_t *seg_offsets,
                                           uint64_t n_segments, double tau, int location, oi_social_counters *out) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    if (n_segments == 0) return OI_OK;
    OI_REQUIRE(seg_offsets && out, "segmented summary: null buffer");
    OI_REQUIRE((polarity && speculative) || n_posts == 0, "segmented summary: null buffer");
    OI_REQUIRE(location == OI_HOST || location == OI_DEVICE, "segmented summary: bad location");
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    if (location == OI_DEVICE)
        return oi_launch_social_summary_segmented(ctx, sources, polarity, speculative, n_posts, seg_offsets, n_segments, tau, out);
    for (uint64_t s = 0; s < n_segments; ++s)
        OI_REQUIRE(seg_offsets[s] <= seg_offsets[s + 1], "segmented summary: segment %llu has offsets %llu > %llu",
                   (unsigned long long)s, (unsigned long long)seg_offsets[s], (unsigned long long)seg_offsets[s + 1]);
    if (seg_offsets[n_segments] > n_posts) { // the analyzer handed back fewer signals than the segments cover (speculation_engine.rs:29-34)
        oi_set_error("segments cover %llu posts, %llu signals given", (unsigned long long)seg_offsets[n_segments],
                     (unsigned long long)n_posts);
        return OI_ERR_ANALYZER_MISMATCH;
    }
    hipStream_t st = ctx->stream;
    // [polarity f64 | segment offsets u64 | speculative u8 | sources u8] in one buffer, one DMA for a call under 1 MB (a
    // scan_watchlist call: a few thousand signals); the records come back in one
    const size_t pb = sizeof(double) * n_posts, gb = sizeof(uint64_t) * (n_segments + 1);
    const size_t off_g = pb, off_f = off_g + gb, off_s = off_f + ((n_posts + 15) & ~(size_t)15), in_bytes = off_s + n_posts + 16;
    const size_t out_bytes = sizeof(oi_social_counters) * n_segments;
    const bool pinned = in_bytes <= OI_PINNED_STAGE_MAX && out_bytes <= OI_PINNED_STAGE_MAX;
    DevBuf &si = ctx->buf("sum_seg_in"), &ob = ctx->buf("sum_seg_out");
    OI_CHECK(si.ensure(in_bytes));
    OI_CHECK(ob.ensure(out_bytes));
    uint8_t *d = si.as<uint8_t>();
    if (pinned) {
        OI_CHECK(ctx->pin_in.ensure(in_bytes));
        OI_CHECK(ctx->pin_out.ensure(out_bytes));
        uint8_t *h = ctx->pin_in.as<uint8_t>();
        if (n_posts) {
            memcpy(h, polarity, pb);
            memcpy(h + off_f, speculative, n_posts);
            if (sources) memcpy(h + off_s, sources, n_posts);
        }
        memcpy(h + off_g, seg_offsets, gb);
        OI_HIP_CHECK(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st));
    } else {
        if (n_posts) {
            OI_HIP_CHECK(hipMemcpyAsync(d, polarity, pb, hipMemcpyHostToDevice, st));
            OI_HIP_CHECK(hipMemcpyAsync(d + off_f, speculative, n_posts, hipMemcpyHostToDevice, st));
            if (sources) OI_HIP_CHECK(hipMemcpyAsync(d + off_s, sources, n_posts, hipMemcpyHostToDevice, st));
        }
        OI_HIP_CHECK(hipMemcpyAsync(d + off_g, seg_offsets, gb, hipMemcpyHostToDevice, st));
    }
    OI_CHECK(oi_launch_social_summary_segmented(ctx, sources && n_posts ? d + off_s : nullptr, reinterpret_cast<const double *>(d),
                                                d + off_f, n_posts, reinterpret_cast<const uint64_t *>(d + off_g), n_segments, tau,
                                                ob.as<oi_social_counters>()));
    if (pinned) {
        OI_HIP_CHECK(hipMemcpyAsync(ctx->pin_out.p, ob.p, out_bytes, hipMemcpyDeviceToHost, st));
        OI_HIP_CHECK(hipStreamSynchronize(st));
        memcpy(out, ctx->pin_out.p, out_bytes);
    } else {
        OI_HIP_CHECK(hipMemcpyAsync(out, ob.p, out_bytes, hipMemcpyDeviceToHost, st));
        OI_HIP_CHECK(hipStreamSynchronize(st));
    }
    return OI_OK;
}

// LexiconAnalyzer::analyze over the pooled posts of many tickers + every ticker's social_summary sums: two launches on the
// ctx stream, nothing copied, nothing synchronised.
extern "C" int oi_lexicon_scan_segments_device(oi_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets, uint64_t n,
                                               uint64_t blob_bytes, const uint8_t *d_sources, const uint64_t *d_seg_offsets,
                                               uint64_t n_segments, double tau, double *d_pol, uint8_t *d_spec,
                                               oi_social_counters *d_out) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    if (n_segments == 0) return OI_OK;
    OI_REQUIRE(d_seg_offsets && d_out, "scan segments: null buffer");
    OI_REQUIRE(n == 0 || (d_offsets && (d_blob || blob_bytes == 0)), "scan segments: null buffer");
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    if (n) {
        if (!d_pol) { // the signals are wanted only as the reduction's input: the ctx's own workspace
            DevBuf &p = ctx->buf("lex_pol");
            OI_CHECK(p.ensure(sizeof(double) * n));
            d_pol = p.as<double>();
        }
        if (!d_spec) {
            DevBuf &f = ctx->buf("lex_spec");
            OI_CHECK(f.ensure(n));
            d_spec = f.as<uint8_t>();
        }
        OI_CHECK(oi_launch_lexicon(ctx, d_blob, d_offsets, n, blob_bytes, d_pol, d_spec));
    }
    return oi_launch_social_summary_segmented(ctx, d_sources, d_pol, d_spec, n, d_seg_offsets, n_segments, tau, d_out);
}

// ---------------------------------------------------------------- index
static std::atomic<uint64_t> g_index_uid{1};

extern "C" int oi_index_create(oi_ctx *ctx, uint64_t n_docs, uint32_t dim, uint32_t vocab, uint32_t doc_id_base,
                               oi_index **out) {
    if (!ctx || !out) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    *out = nullptr;
    OI_REQUIRE(n_docs > 0 && n_docs + doc_id_base <= 0xFFFFFFFFull, "index: doc ids must fit in 32 bits");
    OI_REQUIRE(dim % 4 == 0 && dim >= 4 && dim <= OI_MAX_DIM, "index: dim=%u must be a multiple of 4 in [4,%u]", dim,
               OI_MAX_DIM);
    OI_REQUIRE(vocab > 0, "index: vocab must be > 0");
    oi_index *idx = new oi_index();
    idx->uid = g_index_uid.fetch_add(1);
    idx->ctx = ctx;
    ctx->refs.fetch_add(1);
    idx->n_docs = n_docs;
    idx->dim = dim;
    idx->vocab = vocab;
    idx->doc_id_base = doc_id_base;
    *out = idx;
    return OI_OK;
}

// A second handle on a finalized index, bound to another context (its own stream and workspaces) of the same device:
// searches through the two handles can be in flight at the same time.  The view borrows every buffer.
extern "C" int oi_index_view(oi_index *src, oi_ctx *ctx, oi_index **out) {
    if (!src || !ctx || !out) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    *out = nullptr;
    OI_REQUIRE(ctx != src->ctx, "index view: give it a context of its own (the point is a second stream and second workspaces)");
    OI_REQUIRE(ctx->device == src->ctx->device, "index view: context on device %d, index on device %d", ctx->device, src->ctx->device);
    std::lock_guard<std::mutex> g(src->ctx->mu); // the source is not being built or searched while it is aliased
    if (!src->finalized || (!src->rows && !src->rows_bf16)) { oi_set_error("index view: the source must have rows and be finalized"); return OI_ERR_STATE; }
    oi_index *v = new oi_index();
    v->uid = g_index_uid.fetch_add(1);
    v->ctx = ctx;
    ctx->refs.fetch_add(1);
    v->src = src;
    src->refs.fetch_add(1); // the buffers it borrows live until the last handle on them is gone
    v->is_view = true;
    v->n_docs = src->n_docs; v->dim = src->dim; v->vocab = src->vocab; v->doc_id_base = src->doc_id_base;
    v->rows = src->rows; v->rows_bf16 = src->rows_bf16; // rows_owned / rows_bf16_owned stay false
    v->screen_ok = src->screen_ok; v->screen_copy_policy = src->screen_copy_policy;
    v->forward_set = src->forward_set; v->finalized = true;
    v->total_tokens = src->total_tokens; v->n_postings = src->n_postings; v->n_blocks = src->n_blocks; v->n_win = src->n_win;
    v->avgdl = src->avgdl; v->max_query_terms = src->max_query_terms; v->bm25_mode = src->bm25_mode;
    auto alias = [](DevBuf &dst, const DevBuf &from) { dst.p = from.p; dst.cap = from.cap; dst.borrowed = from.p != nullptr; };
    alias(v->max_row_norm, src->max_row_norm); alias(v->screen_copy, src->screen_copy); alias(v->screen_i8, src->screen_i8);
    alias(v->screen_i8r, src->screen_i8r);
    alias(v->uniq_keys, src->uniq_keys); alias(v->tf, src->tf); alias(v->doc_len, src->doc_len); alias(v->df_local, src->df_local);
    alias(v->postings, src->postings); alias(v->cell_start, src->cell_start); alias(v->idf, src->idf);
    alias(v->impact_floor, src->impact_floor);
    v->n_long = src->n_long; alias(v->long_list, src->long_list); alias(v->long_bitmap, src->long_bitmap);
    alias(v->fwd_terms, src->fwd_terms); alias(v->fwd_offsets, src->fwd_offsets);
    alias(v->doc_attrs, src->doc_attrs); // (never reallocated: the view sees later in-place updates of the source's)
    alias(v->signals, src->signals);     // (likewise)
    *out = v;
    return OI_OK;
}

// Drops one reference; the last one frees the buffers (a source index with live views stays until they are gone),
// then lets go of the source (a view) and of the ctx.
static void index_release(oi_index *idx) {
    if (idx->refs.fetch_sub(1) != 1) return;
    oi_ctx *ctx = idx->ctx;
    oi_index *src = idx->src;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        graphs_purge(ctx, idx->uid);
        if (idx->rows_owned && idx->rows) (void)hipFree(idx->rows);
        if (idx->rows_bf16_owned && idx->rows_bf16) (void)hipFree(idx->rows_bf16);
        idx->uniq_keys.release(); idx->tf.release(); idx->doc_len.release(); idx->df_local.release();
        idx->postings.release(); idx->cell_start.release(); idx->idf.release();
        idx->fwd_terms.release(); idx->fwd_offsets.release(); idx->max_row_norm.release(); idx->screen_copy.release();
        idx->screen_i8.release(); idx->screen_i8r.release();
    }
    delete idx;
    if (src) index_release(src);
    ctx_release(ctx);
}

extern "C" void oi_index_destroy(oi_index *idx) {
    if (!idx) return;
    {   // nothing of this handle's work stays in flight behind the call, whoever frees the buffers in the end
        std::lock_guard<std::mutex> g(idx->ctx->mu);
        (void)hipSetDevice(idx->ctx->device);
        (void)hipStreamSynchronize(idx->ctx->stream);
        if (idx->ctx->side_stream) (void)hipStreamSynchronize(idx->ctx->side_stream);
    }
    index_release(idx);
}

// The bf16 screening copy of an f32 corpus (include/openintel_hip.h: oi_index_set_screen_copy).  Called with the ctx mutex
// held, at finalize and whenever the rows or the policy of a finalized index change.  AUTO: only when the corpus can be
// screened at all and n x d x 2 bytes are at most a quarter (OI_SCREEN_COPY_MAX_FRAC) of the device memory free right now.
static int default_screen_copy_policy() {
    static const int p = [] {
        const char *e = getenv("OI_SCREEN_COPY");
        return !e ? OI_SCREEN_COPY_AUTO : strcmp(e, "never") == 0 ? OI_SCREEN_COPY_NEVER : strcmp(e, "always") == 0 ? OI_SCREEN_COPY_ALWAYS
                                                                                                                  : OI_SCREEN_COPY_AUTO;
    }();
    return p;
}
static int apply_screen_copy_policy(oi_index *idx) {
    oi_ctx *ctx = idx->ctx;
    if (idx->is_view) return OI_OK;
    const int policy = idx->screen_copy_policy < 0 ? default_screen_copy_policy() : idx->screen_copy_policy;
    if (policy == OI_SCREEN_COPY_NEVER || !oi_index_screenable(idx)) {
        if (idx->screen_copy.p || idx->screen_i8.p || idx->screen_i8r.p) {
            OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            idx->screen_copy.release();
            idx->screen_i8.release();
            idx->screen_i8r.release();
        }
        return OI_OK;
    }
    if (idx->screen_copy.p) return OI_OK; // (set_embeddings releases the copies of the previous rows)
    // The bf16 copy and, in front of it, the int8 copy of the first screening tier (cosine_screen_i8.hip): AUTO makes both when
    // both fit the budget, the bf16 one alone when only it does; and behind the int8 copy its residual plane
    // (screen_i8_residual.hip, the int8 copy's size once more) when all three fit -- the first to be left out
    const size_t bytes = sizeof(uint16_t) * (size_t)idx->n_docs * idx->dim + 64;
    const size_t bytes_i8 = oi_screen_i8_bytes(idx->n_docs, idx->dim);
    bool with_i8 = true, with_i8r = true;
    if (policy == OI_SCREEN_COPY_AUTO) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return OI_OK; // no figure, no copy
        static const double frac = [] {
            const char *e = getenv("OI_SCREEN_COPY_MAX_FRAC");
            const double f = e ? atof(e) : 0.25;
            return f > 0.0 && f <= 1.0 ? f : 0.25;
        }();
        if ((double)bytes > frac * (double)free_b) return OI_OK;
        with_i8 = (double)(bytes + bytes_i8) <= frac * (double)free_b;
        with_i8r = (double)(bytes + 2 * bytes_i8) <= frac * (double)free_b;
    }
    OI_CHECK(idx->screen_copy.ensure(bytes));
    OI_CHECK(oi_launch_make_screen_copy(ctx, idx->rows, idx->n_docs, idx->dim, idx->screen_copy.as<uint16_t>()));
    if (with_i8) {
        OI_CHECK(idx->screen_i8.ensure(bytes_i8));
        OI_CHECK(oi_launch_make_screen_i8(ctx, idx->rows, idx->n_docs, idx->dim, idx->n_long ? idx->long_bitmap.as<uint32_t>() : nullptr,
                                          idx->screen_i8.as<uint8_t>()));
        if (with_i8r) {
            OI_CHECK(idx->screen_i8r.ensure(bytes_i8));
            OI_CHECK(oi_launch_make_screen_i8_residual(ctx, idx->rows, idx->n_docs, idx->dim, idx->n_long ? idx->long_bitmap.as<uint32_t>() : nullptr,
                                                       idx->screen_i8.as<uint8_t>(), idx->screen_i8r.as<uint8_t>()));
        }
    }
    OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return OI_OK;
}

// Not part of the C ABI: the residual plane of an index, for the tests.  drop != 0 frees it (the index is then what the AUTO budget
// makes when only two copies fit); otherwise the n x dim bytes, the n {t_r, e2_r} pairs and e2_max are copied to the host
// pointers that are not null.  *bytes_out: the plane's allocation, 0 = the index holds none.
extern "C" int oi_internal_residual_plane(oi_index *idx, int drop, uint8_t *rows_out, float *meta_out, float *e2max_out, uint64_t *bytes_out) {
    if (!idx) { oi_set_error("null index"); return OI_ERR_INVALID_ARG; }
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (drop) {
        OI_REQUIRE(!idx->is_view, "index view: read-only");
        OI_REQUIRE(idx->refs.load() == 1, "residual plane: the index has live views that alias it");
        g_oi_ws_epoch.fetch_add(1);
        idx->screen_i8r.release();
    }
    if (bytes_out) *bytes_out = idx->screen_i8r.p ? (uint64_t)idx->screen_i8r.cap : 0;
    if (!idx->screen_i8r.p || drop) return OI_OK;
    const uint8_t *p = idx->screen_i8r.as<uint8_t>();
    const size_t n = idx->n_docs, mo = oi_screen_i8_meta_offset(n, idx->dim);
    if (rows_out && n) OI_HIP_CHECK(hipMemcpy(rows_out, p, n * idx->dim, hipMemcpyDeviceToHost));
    if (meta_out && n) OI_HIP_CHECK(hipMemcpy(meta_out, p + mo, 8 * n, hipMemcpyDeviceToHost));
    if (e2max_out) OI_HIP_CHECK(hipMemcpy(e2max_out, p + mo + 8 * (n + 64), 4, hipMemcpyDeviceToHost)); // (behind the 64 padding rows: I8S_PAD_ROWS)
    return OI_OK;
}

// Not part of the C ABI: the long rows of an index (local row numbers) in the order of its long_list, for the tests -- the order
// is that of pf_row_norm_class_kernel's atomics, and pf_rescore_kernel packs the passing long rows of a filtered search by their
// position in it.  *n_out: idx->n_long; rows_out (may be null): room for OI_LONG_ROWS_MAX words, n_long of them written.
extern "C" int oi_internal_long_list(oi_index *idx, uint32_t *n_out, uint32_t *rows_out) {
    if (!idx || !n_out) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *n_out = idx->n_long;
    if (rows_out && idx->n_long && idx->long_list.p)
        OI_HIP_CHECK(hipMemcpy(rows_out, idx->long_list.p, sizeof(uint32_t) * idx->n_long, hipMemcpyDeviceToHost));
    return OI_OK;
}

// Not part of the C ABI: the BM25 structures of a finalized index (or of a view of one), for the tests.  Always: the number of
// postings, the windows per term and avgdl.  Copied to the host pointers that are not null: the postings as n_postings pairs
// {u32 doc_in_block, f32 impact}, cell_start [vocab * n_win + 1], idf [vocab], the impact floors [vocab * OI_BM25_FLOOR_RANKS]
// and doc_len [n_docs].  An index without a posting has no cell table (oi_bm25_stage_forward builds none, no kernel reads
// one): every run is empty, cell_start is given as zeros.
extern "C" int oi_internal_bm25_index(oi_index *idx, uint64_t *n_postings_out, uint32_t *n_win_out, float *avgdl_out, void *postings_out,
                                      uint32_t *cell_start_out, float *idf_out, uint32_t *floors_out, uint32_t *doc_len_out) {
    if (!idx) { oi_set_error("null index"); return OI_ERR_INVALID_ARG; }
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!idx->finalized) { oi_set_error("bm25 index: the index is not finalized"); return OI_ERR_STATE; }
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (n_postings_out) *n_postings_out = idx->n_postings;
    if (n_win_out) *n_win_out = idx->n_win;
    if (avgdl_out) *avgdl_out = idx->avgdl;
    const size_t np = idx->n_postings, cells = (size_t)idx->vocab * idx->n_win + 1;
    if (postings_out && np) OI_HIP_CHECK(hipMemcpy(postings_out, idx->postings.p, 8 * np, hipMemcpyDeviceToHost));
    if (cell_start_out) {
        if (np) OI_HIP_CHECK(hipMemcpy(cell_start_out, idx->cell_start.p, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost));
        else memset(cell_start_out, 0, sizeof(uint32_t) * cells);
    }
    if (idf_out) OI_HIP_CHECK(hipMemcpy(idf_out, idx->idf.p, sizeof(float) * idx->vocab, hipMemcpyDeviceToHost));
    if (floors_out)
        OI_HIP_CHECK(hipMemcpy(floors_out, idx->impact_floor.p, sizeof(uint32_t) * (size_t)idx->vocab * OI_BM25_FLOOR_RANKS, hipMemcpyDeviceToHost));
    if (doc_len_out && idx->n_docs) OI_HIP_CHECK(hipMemcpy(doc_len_out, idx->doc_len.p, sizeof(uint32_t) * (size_t)idx->n_docs, hipMemcpyDeviceToHost));
    return OI_OK;
}

// Not part of the C ABI: the int8 route's query staging and its residual rescreen over the caller's keys, for the tests
// (tests/test_gpu_residual_rescreen_edges.py).  An index that holds both int8 planes, or a view of one.  The two product launchers
// run unchanged on the ctx stream, in workspaces of this call's own ("rescreen_probe_*": none of a search's): oi_launch_screen_stage_i8
// over the B host queries [B, dim] with the index's max_row_norm, int8 copy and residual plane, then oi_launch_rescreen_residual
// over a pool whose keys [B, stride] and counts [B] are the caller's and whose carry_cap is `cap` (<= stride: the kernel clamps a
// count to it).  Copied back to the host pointers that are not null: the WHOLE key block (in place), the staged qi8 block
// [2][n_padded][dim] (h then l, n_padded = B rounded up to 32), qf [4][n_padded] (a, |q^|, c_q, m2), eps2_residual [B], the gate
// word, and the three scalars the staging read: {X = max_row_norm[0], e_max, e2_max}.
extern "C" int oi_internal_residual_rescreen(oi_index *idx, const float *queries, uint32_t B, uint64_t *keys, const uint32_t *counts,
                                             uint64_t stride, uint32_t cap, int8_t *qi8_out, float *qf_out, float *eps2r_out,
                                             uint32_t *gate_out, float *scalars_out) {
    if (!idx || !queries || !keys || !counts) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(B >= 1 && B <= 4096, "residual rescreen probe: n_queries=%u outside [1,4096]", B);
    OI_REQUIRE(stride >= 1 && (uint64_t)B * stride <= (1u << 24) && cap >= 1 && cap <= stride,
               "residual rescreen probe: stride %llu (at most 2^24 keys in all) or cap %u outside [1, stride]", (unsigned long long)stride, cap);
    OI_REQUIRE(idx->dim == 384 || idx->dim == 768, "residual rescreen probe: dim %u not instantiated (384, 768)", idx->dim);
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_REQUIRE(idx->n_docs >= 1 && idx->max_row_norm.p && idx->screen_i8.p && idx->screen_i8r.p,
               "residual rescreen probe: the index does not hold both int8 planes");
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t dim = idx->dim, n_padded = (B + 31u) & ~31u;
    const uint64_t n = idx->n_docs;
    const size_t q_bytes = sizeof(float) * (size_t)B * dim, key_bytes = sizeof(uint64_t) * (size_t)B * stride;
    const size_t qi8_bytes = ((2 * (size_t)n_padded * dim) + 255) & ~(size_t)255, qf_bytes = sizeof(float) * 4 * (size_t)n_padded;
    DevBuf &qv = ctx->buf("rescreen_probe_q"), &qb = ctx->buf("rescreen_probe_q_bf16"), &qs = ctx->buf("rescreen_probe_q_i8"),
           &ws = ctx->buf("rescreen_probe_state"), &pk = ctx->buf("rescreen_probe_keys");
    OI_CHECK(qv.ensure(q_bytes));
    OI_CHECK(qb.ensure(sizeof(uint16_t) * (size_t)(n_padded + 64) * dim));
    OI_CHECK(qs.ensure(qi8_bytes + qf_bytes));
    OI_CHECK(ws.ensure(sizeof(uint32_t) * (2 * (size_t)B + 4))); // counts[B] eps2[B] gate[4]
    OI_CHECK(pk.ensure(key_bytes));
    uint32_t *d_cnt = ws.as<uint32_t>();
    float *d_eps2 = reinterpret_cast<float *>(d_cnt + B);
    uint32_t *d_gate = d_cnt + 2 * (size_t)B;
    int8_t *d_qi8 = qs.as<int8_t>();
    float *d_qf = reinterpret_cast<float *>(qs.as<unsigned char>() + qi8_bytes);
    OI_HIP_CHECK(hipMemcpyAsync(qv.p, queries, q_bytes, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemcpyAsync(pk.p, keys, key_bytes, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemsetAsync(ws.p, 0, sizeof(uint32_t) * (2 * (size_t)B + 4), st));
    OI_HIP_CHECK(hipMemcpyAsync(d_cnt, counts, sizeof(uint32_t) * (size_t)B, hipMemcpyHostToDevice, st));
    // (as search.hip stages the residual tail: the residual tier's margin over the bf16 screen's, in one array)
    OI_CHECK(oi_launch_screen_stage_i8(ctx, qv.as<float>(), B, dim, idx->max_row_norm.as<uint32_t>(), idx->screen_i8.as<uint8_t>(), n, d_qi8, d_qf,
                                       d_gate, qb.as<uint16_t>(), d_eps2, idx->screen_i8r.as<uint8_t>(), d_eps2));
    PoolView P{};
    P.keys = pk.as<uint64_t>(); P.carry_cnt = d_cnt; P.stride = stride; P.carry_cap = cap;
    OI_CHECK(oi_launch_rescreen_residual(ctx, idx->screen_i8r.as<uint8_t>(), idx->screen_i8.as<uint8_t>(), n, dim, idx->doc_id_base, d_qi8, d_qf, B, P));
    OI_HIP_CHECK(hipMemcpyAsync(keys, pk.p, key_bytes, hipMemcpyDeviceToHost, st));
    if (qi8_out) OI_HIP_CHECK(hipMemcpyAsync(qi8_out, d_qi8, 2 * (size_t)n_padded * dim, hipMemcpyDeviceToHost, st));
    if (qf_out) OI_HIP_CHECK(hipMemcpyAsync(qf_out, d_qf, qf_bytes, hipMemcpyDeviceToHost, st));
    if (eps2r_out) OI_HIP_CHECK(hipMemcpyAsync(eps2r_out, d_eps2, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (gate_out) OI_HIP_CHECK(hipMemcpyAsync(gate_out, d_gate, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (scalars_out) {
        const size_t emax_at = oi_screen_i8_meta_offset(n, dim) + 8 * ((size_t)n + 64); // (behind the 64 padding rows: I8S_PAD_ROWS)
        OI_HIP_CHECK(hipMemcpyAsync(scalars_out, idx->max_row_norm.p, 4, hipMemcpyDeviceToHost, st));
        OI_HIP_CHECK(hipMemcpyAsync(scalars_out + 1, idx->screen_i8.as<uint8_t>() + emax_at, 4, hipMemcpyDeviceToHost, st));
        OI_HIP_CHECK(hipMemcpyAsync(scalars_out + 2, idx->screen_i8r.as<uint8_t>() + emax_at, 4, hipMemcpyDeviceToHost, st));
    }
    OI_HIP_CHECK(hipStreamSynchronize(st));
    return OI_OK;
}

extern "C" int oi_index_set_screen_copy(oi_index *idx, int policy) {
    if (!idx) { oi_set_error("null index"); return OI_ERR_INVALID_ARG; }
    if (idx->is_view) { oi_set_error("index view: read-only (set the policy on the index it was taken from)"); return OI_ERR_STATE; }
    OI_REQUIRE(policy == OI_SCREEN_COPY_AUTO || policy == OI_SCREEN_COPY_NEVER || policy == OI_SCREEN_COPY_ALWAYS,
               "oi_index_set_screen_copy: unknown policy %d", policy);
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    idx->screen_copy_policy = policy;
    if (!idx->finalized) return OI_OK; // applied by finalize
    g_oi_ws_epoch.fetch_add(1);        // captured query calls hold (or lack) the copy's pointer
    return apply_screen_copy_policy(idx);
}

extern "C" int oi_index_bytes(oi_index *idx, uint64_t *rows_owned, uint64_t *screen_copy, uint64_t *bm25) {
    if (!idx) { oi_set_error("null index"); return OI_ERR_INVALID_ARG; }
    std::lock_guard<std::mutex> g(idx->ctx->mu);
    if (rows_owned)
        *rows_owned = (idx->rows_owned ? sizeof(float) * (uint64_t)idx->n_docs * idx->dim : 0) +
                      (idx->rows_bf16_owned ? sizeof(uint16_t) * (uint64_t)idx->n_docs * idx->dim : 0);
    if (screen_copy)
        *screen_copy = (idx->screen_copy.p && !idx->screen_copy.borrowed ? (uint64_t)idx->screen_copy.cap : 0) +
                       (idx->screen_i8.p && !idx->screen_i8.borrowed ? (uint64_t)idx->screen_i8.cap : 0) +
                       (idx->screen_i8r.p && !idx->screen_i8r.borrowed ? (uint64_t)idx->screen_i8r.cap : 0);
    if (bm25) {
        uint64_t b = 0;
        for (const DevBuf *d : {&idx->uniq_keys, &idx->tf, &idx->doc_len, &idx->df_local, &idx->postings, &idx->cell_start, &idx->idf,
                                &idx->impact_floor, &idx->fwd_terms, &idx->fwd_offsets})
            if (d->p && !d->borrowed) b += d->cap;
        *bm25 = b;
    }
    return OI_OK;
}

extern "C" int oi_index_set_embeddings(oi_index *idx, float *rows, int location, int normalize) {
    if (!idx || !rows) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    if (idx->is_view) { oi_set_error("index view: read-only (set the data on the index it was taken from)"); return OI_ERR_STATE; }
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    // captured query calls (oi_set_graph_replay) hold the OLD rows pointer -- on this ctx and on every view's: stale from here
    // on (the epoch is process-wide; a raw hipMalloc / hipFree or a caller's pointer does not bump it by itself)
    g_oi_ws_epoch.fetch_add(1);
    if (idx->rows_owned && idx->rows) { (void)hipFree(idx->rows); idx->rows = nullptr; idx->rows_owned = false; }
    if (idx->rows_bf16_owned && idx->rows_bf16) (void)hipFree(idx->rows_bf16);
    idx->rows_bf16 = nullptr; idx->rows_bf16_owned = false;
    idx->screen_copy.release(); // a copy of the previous rows
    idx->screen_i8.release();
    idx->screen_i8r.release();
    const size_t bytes = (size_t)idx->n_docs * idx->dim * sizeof(float);
    if (location == OI_DEVICE) {
        OI_REQUIRE(((uintptr_t)rows & 15u) == 0, "index: embedding matrix must be 16-byte aligned");
        idx->rows = rows;
    } else {
        void *p = nullptr;
        OI_HIP_CHECK(hipMalloc(&p, bytes));
        idx->rows = reinterpret_cast<float *>(p);
        idx->rows_owned = true;
        OI_HIP_CHECK(hipMemcpyAsync(idx->rows, rows, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    if (normalize) OI_CHECK(oi_launch_l2_normalize(ctx, idx->rows, idx->n_docs, idx->dim));
    // the bf16 screen's error bound needs max |row| and max |bf16(row) - row| (cosine_prefilter.hip): one more pass
    // over the rows, now
    OI_CHECK(idx->max_row_norm.ensure(64));
    OI_CHECK(oi_launch_row_norm_max(ctx, idx->rows, idx->n_docs, idx->dim, idx->max_row_norm.as<uint32_t>()));
    OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    idx->n_long = 0;
    idx->long_list.release(); idx->long_bitmap.release();
    {   // a corpus whose largest norm is not finite, or so large that bf16 products could overflow, is never screened
        struct { float X, E; double sx2, se2; } mx = {0.f, 0.f, 0.0, 0.0}; // X = max |row|, E = max |bf16(row) - row|, sums of squares
        OI_HIP_CHECK(hipMemcpy(&mx, idx->max_row_norm.p, 24, hipMemcpyDeviceToHost));
        idx->screen_ok = mx.X < 1.0e15f && mx.E < 1.0e15f; // false for NaN
        // Two classes (cosine_prefilter.hip): when the largest norms stand out from the corpus (> 1.5 x the RMS) and the rows
        // responsible are few, they are set aside -- always rescored, never part of the screen's thresholds -- and the margin
        // is built from the maxima over the REST.  A normalised corpus never gets here (no second pass over the rows).
        const uint64_t n = idx->n_docs;
        if (idx->screen_ok && n > 4 * OI_LONG_ROWS_MAX) {
            const float X0 = 1.5f * (float)std::sqrt(mx.sx2 / (double)n), E0 = 1.5f * (float)std::sqrt(mx.se2 / (double)n);
            if ((mx.X > X0 || mx.E > E0) && X0 > 0.f && E0 > 0.f) {
                DevBuf cls;
                OI_CHECK(cls.ensure(16));
                OI_CHECK(idx->long_list.ensure(sizeof(uint32_t) * OI_LONG_ROWS_MAX));
                OI_CHECK(idx->long_bitmap.ensure(((n + 31) / 32) * 4));
                OI_CHECK(oi_launch_row_norm_classes(ctx, idx->rows, n, idx->dim, X0, E0, cls.as<uint32_t>(), idx->long_bitmap.as<uint32_t>(),
                                                    idx->long_list.as<uint32_t>(), OI_LONG_ROWS_MAX));
                uint32_t h[4] = {0, 0, 0, 0};
                OI_HIP_CHECK(hipMemcpyAsync(h, cls.p, 16, hipMemcpyDeviceToHost, ctx->stream));
                OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
                if (h[2] >= 1 && h[2] <= OI_LONG_ROWS_MAX) {
                    idx->n_long = h[2];
                    OI_HIP_CHECK(hipMemcpy(idx->max_row_norm.p, h, 8, hipMemcpyHostToDevice)); // the maxima over the other rows
                } else {
                    idx->long_list.release(); idx->long_bitmap.release(); // too many to set aside: one class, the corpus maxima
                }
            }
        }
    }
    if (idx->finalized) OI_CHECK(apply_screen_copy_policy(idx)); // new rows under a finalized index: a new copy, now
    return OI_OK;
}

extern "C" int oi_index_set_embeddings_bf16(oi_index *idx, const uint16_t *rows, int location) {
    if (!idx || !rows) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    if (idx->is_view) { oi_set_error("index view: read-only (set the data on the index it was taken from)"); return OI_ERR_STATE; }
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    // captured query calls (oi_set_graph_replay) hold the OLD rows pointer -- on this ctx and on every view's: stale from here
    // on (the epoch is process-wide; a raw hipMalloc / hipFree or a caller's pointer does not bump it by itself)
    g_oi_ws_epoch.fetch_add(1);
    OI_REQUIRE(oi_cosine_bf16_supported(idx->dim), "index: a bf16 corpus needs dim 384, 768 or 1024 (got %u)", idx->dim);
    if (idx->rows_owned && idx->rows) (void)hipFree(idx->rows);
    idx->rows = nullptr; idx->rows_owned = false;
    idx->screen_copy.release(); // (a copy of f32 rows that are gone)
    idx->screen_i8.release();
    idx->screen_i8r.release();
    if (idx->rows_bf16_owned && idx->rows_bf16) (void)hipFree(idx->rows_bf16);
    idx->rows_bf16 = nullptr; idx->rows_bf16_owned = false;
    const size_t bytes = (size_t)idx->n_docs * idx->dim * sizeof(uint16_t);
    if (location == OI_DEVICE) {
        OI_REQUIRE(((uintptr_t)rows & 15u) == 0, "index: embedding matrix must be 16-byte aligned");
        idx->rows_bf16 = const_cast<uint16_t *>(rows);
    } else {
        void *p = nullptr;
        OI_HIP_CHECK(hipMalloc(&p, bytes));
        idx->rows_bf16 = reinterpret_cast<uint16_t *>(p);
        idx->rows_bf16_owned = true;
        OI_HIP_CHECK(hipMemcpyAsync(idx->rows_bf16, rows, bytes, hipMemcpyHostToDevice, ctx->stream));
        OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return OI_OK;
}

extern "C" int oi_index_set_forward(oi_index *idx, const uint32_t *term_ids, const uint64_t *doc_offsets,
                                    int location) {
    if (!idx || !doc_offsets) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    if (idx->is_view) { oi_set_error("index view: read-only (set the data on the index it was taken from)"); return OI_ERR_STATE; }
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    if (location == OI_DEVICE) return oi_bm25_stage_forward(idx, term_ids, doc_offsets);
    const uint64_t total = doc_offsets[idx->n_docs];
    DevBuf t, o;
    OI_CHECK(t.ensure(sizeof(uint32_t) * (total ? total : 1)));
    OI_CHECK(o.ensure(sizeof(uint64_t) * (idx->n_docs + 1)));
    if (total) OI_HIP_CHECK(hipMemcpyAsync(t.p, term_ids, sizeof(uint32_t) * total, hipMemcpyHostToDevice, ctx->stream));
    OI_HIP_CHECK(hipMemcpyAsync(o.p, doc_offsets, sizeof(uint64_t) * (idx->n_docs + 1), hipMemcpyHostToDevice,
                                ctx->stream));
    int rc = oi_bm25_stage_forward(idx, t.as<uint32_t>(), o.as<uint64_t>());
    (void)hipStreamSynchronize(ctx->stream);
    t.release();
    o.release();
    return rc;
}

extern "C" int oi_index_set_max_query_terms(oi_index *idx, uint32_t max_terms) {
    if (!idx) { oi_set_error("null index"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(max_terms >= 1 && max_terms <= 1024, "max_query_terms=%u outside [1,1024]", max_terms);
    std::lock_guard<std::mutex> g(idx->ctx->mu);
    idx->max_query_terms = max_terms;
    return OI_OK;
}

extern "C" int oi_index_long_rows(oi_index *idx, uint32_t *n_out) {
    if (!idx || !n_out) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    *n_out = idx->n_long;
    return OI_OK;
}

extern "C" int oi_index_set_bm25_mode(oi_index *idx, int mode) {
    if (!idx) { oi_set_error("null index"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(mode >= 0 && mode <= 4, "bm25 mode %d outside [0,4]", mode);
    std::lock_guard<std::mutex> g(idx->ctx->mu);
    idx->bm25_mode = mode;
    return OI_OK;
}

// {group, stamp} per local row, interleaved (one 8-byte load on a kernel's hit path).  The buffer is allocated by the first
// call and only overwritten after that (stream-ordered on the ctx): views alias it and see every later update.
extern "C" int oi_index_set_doc_attrs(oi_index *idx, const uint32_t *group, const uint32_t *stamp, int location) {
    if (!idx) { oi_set_error("null index"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(location == OI_HOST || location == OI_DEVICE, "set_doc_attrs: bad location %d", location);
    if (idx->is_view) { oi_set_error("set_doc_attrs: a view's attributes are its source's"); return OI_ERR_STATE; }
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    const uint64_t n = idx->n_docs;
    if (n == 0) return OI_OK;
    if (!idx->doc_attrs.p) OI_CHECK(idx->doc_attrs.ensure(sizeof(uint32_t) * 2 * (size_t)n));
    uint32_t *d = idx->doc_attrs.as<uint32_t>();
    hipStream_t st = ctx->stream;
    if (location == OI_HOST) {
        std::vector<uint32_t> h(2 * (size_t)n, 0u);
        for (uint64_t i = 0; i < n; ++i) {
            if (group) h[2 * i] = group[i];
            if (stamp) h[2 * i + 1] = stamp[i];
        }
        OI_HIP_CHECK(hipMemcpyAsync(d, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        OI_HIP_CHECK(hipStreamSynchronize(st));
        return OI_OK;
    }
    // device arrays: two strided copies into the interleaved buffer (a NULL array: zeros)
    const uint32_t *src[2] = {group, stamp};
    for (int c = 0; c < 2; ++c) {
        if (src[c]) OI_HIP_CHECK(hipMemcpy2DAsync(d + c, 8, src[c], 4, 4, n, hipMemcpyDeviceToDevice, st));
        else OI_HIP_CHECK(hipMemset2DAsync(d + c, 8, 0, 4, n, st));
    }
    return OI_OK;
}

// One 8-byte signal record per local row (cosine_summary.hip: the pack kernel).  The allocation rules of doc_attrs: made by
// the first call, only overwritten after that (stream-ordered on the ctx), aliased by views.
extern "C" int oi_index_set_signals(oi_index *idx, const double *polarity, const uint8_t *speculative, const uint8_t *sources,
                                    double bull_bear_threshold, int location) {
    OI_REQUIRE(bull_bear_threshold == bull_bear_threshold, "set_signals: bull_bear_threshold is NaN");
    OI_REQUIRE(polarity && speculative, "set_signals: null buffer (%s)", polarity ? "speculative" : "polarity");
    OI_REQUIRE(location == OI_HOST || location == OI_DEVICE, "set_signals: bad location %d", location);
    if (!idx) { oi_set_error("set_signals: null index"); return OI_ERR_INVALID_ARG; }
    if (idx->is_view) { oi_set_error("set_signals: a view's signals are its source's"); return OI_ERR_STATE; }
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    const uint64_t n = idx->n_docs;
    if (n == 0) return OI_OK;
    if (!idx->signals.p) OI_CHECK(idx->signals.ensure(sizeof(uint2) * (size_t)n));
    hipStream_t st = ctx->stream;
    if (location == OI_DEVICE) return oi_launch_pack_signals(ctx, polarity, speculative, sources, n, bull_bear_threshold, idx->signals.as<uint2>());
    DevBuf &w = ctx->buf("signals_io"); // [polarity | speculative | sources]
    const size_t pb = sizeof(double) * (size_t)n;
    OI_CHECK(w.ensure(pb + 2 * (size_t)n));
    uint8_t *d = w.as<uint8_t>();
    OI_HIP_CHECK(hipMemcpyAsync(d, polarity, pb, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemcpyAsync(d + pb, speculative, n, hipMemcpyHostToDevice, st));
    if (sources) OI_HIP_CHECK(hipMemcpyAsync(d + pb + n, sources, n, hipMemcpyHostToDevice, st));
    OI_CHECK(oi_launch_pack_signals(ctx, reinterpret_cast<const double *>(d), d + pb, sources ? d + pb + n : nullptr, n, bull_bear_threshold,
                                    idx->signals.as<uint2>()));
    OI_HIP_CHECK(hipStreamSynchronize(st));
    return OI_OK;
}

extern "C" int oi_index_local_stats(oi_index *idx, uint64_t *total_tokens_out, uint32_t *df_out_host) {
    if (!idx) { oi_set_error("null index"); return OI_ERR_INVALID_ARG; }
    if (idx->is_view) { oi_set_error("index view: read-only (set the data on the index it was taken from)"); return OI_ERR_STATE; }
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!idx->forward_set) { oi_set_error("index: set_forward has not been called"); return OI_ERR_STATE; }
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    if (total_tokens_out) *total_tokens_out = idx->total_tokens;
    if (df_out_host) {
        OI_HIP_CHECK(hipMemcpyAsync(df_out_host, idx->df_local.p, sizeof(uint32_t) * idx->vocab,
                                    hipMemcpyDeviceToHost, ctx->stream));
        OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return OI_OK;
}

extern "C" int oi_index_finalize(oi_index *idx, uint64_t global_n_docs, uint64_t global_total_tokens,
                                 const uint32_t *global_df_host) {
    if (!idx) { oi_set_error("null index"); return OI_ERR_INVALID_ARG; }
    if (idx->is_view) { oi_set_error("index view: read-only (set the data on the index it was taken from)"); return OI_ERR_STATE; }
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!idx->forward_set) { oi_set_error("index: set_forward has not been called"); return OI_ERR_STATE; }
    if (idx->finalized) { oi_set_error("index: already finalized"); return OI_ERR_STATE; }
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    OI_CHECK(oi_bm25_finalize(idx, global_n_docs, global_total_tokens, global_df_host));
    return apply_screen_copy_policy(idx); // the derived structure of the cosine leg, beside the BM25 leg's postings
}

// ---------------------------------------------------------------- search (search.hip: search_lists_device)
namespace {

struct QueryStage {
    const float *qv;
    const uint32_t *qt, *qo;
    const uint4 *filt = nullptr; // a filtered search: the queries' oi_doc_filter (16 B each), device
};

// filters != null (a filtered search): staged with the queries -- in the same DMA for OI_HOST, as given for OI_DEVICE
int stage_queries(oi_index *idx, const float *qv, const uint32_t *qt, const uint32_t *qo, uint32_t B, int location,
                  QueryStage *out, const oi_doc_filter *filters = nullptr) {
    static_assert(sizeof(oi_doc_filter) == sizeof(uint4), "oi_doc_filter is 16 bytes");
    oi_ctx *ctx = idx->ctx;
    if (location == OI_DEVICE) { *out = QueryStage{qv, qt, qo, reinterpret_cast<const uint4 *>(filters)}; return OI_OK; }
    hipStream_t st = ctx->stream;
    const uint32_t nt = qo[B];
    const QueryLayout l(B, idx->dim, nt, filters != nullptr); // one page-locked staging buffer, one DMA
    DevBuf &a = ctx->buf("q_stage");
    OI_CHECK(a.ensure(l.total));
    OI_CHECK(ctx->pin_in.ensure(l.total));
    uint8_t *h = ctx->pin_in.as<uint8_t>();
    memcpy(h, qv, l.vb);
    if (nt) memcpy(h + l.off_t, qt, sizeof(uint32_t) * nt);
    memcpy(h + l.off_o, qo, l.ob);
    if (filters) memcpy(h + l.off_f, filters, sizeof(oi_doc_filter) * (size_t)B);
    OI_HIP_CHECK(hipMemcpyAsync(a.p, h, l.total, hipMemcpyHostToDevice, st));
    uint8_t *d = a.as<uint8_t>();
    *out = QueryStage{reinterpret_cast<const float *>(d), reinterpret_cast<const uint32_t *>(d + l.off_t),
                      reinterpret_cast<const uint32_t *>(d + l.off_o), filters ? reinterpret_cast<const uint4 *>(d + l.off_f) : nullptr};
    return OI_OK;
}

int check_search_args(oi_index *idx, const float *qv, const uint32_t *qo, uint32_t B, uint32_t depth) {
    if (!idx) { oi_set_error("null index"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(qv && qo, "search: null query buffer");
    OI_REQUIRE(B >= 1 && B <= 4096, "search: n_queries=%u outside [1,4096]", B);
    OI_REQUIRE(depth >= 1 && depth <= OI_MAX_DEPTH, "search: depth=%u outside [1,%u]", depth, OI_MAX_DEPTH);
    return OI_OK;
}

// What the five search impls open behind their argument checks: the context locked, the filter state checked (a filtered
// search needs the index's doc attributes), the device set, the queries staged -- in that order.  attrs: the index's doc attributes for a filtered call, null otherwise.
struct SearchCall {
    oi_ctx *ctx = nullptr;
    std::unique_lock<std::mutex> lock;
    QueryStage q;
    const uint2 *attrs = nullptr;
};
int open_search(SearchCall &c, oi_index *idx, const float *qv, const uint32_t *qt, const uint32_t *qo, uint32_t B, int location,
                const oi_doc_filter *filters) {
    c.ctx = idx->ctx;
    c.lock = std::unique_lock<std::mutex>(c.ctx->mu);
    if (filters && !idx->doc_attrs.p) { oi_set_error("filtered search: the index has no doc attributes (oi_index_set_doc_attrs)"); return OI_ERR_STATE; }
    OI_HIP_CHECK(hipSetDevice(c.ctx->device));
    OI_CHECK(stage_queries(idx, qv, qt, qo, B, location, &c.q, filters));
    c.attrs = c.q.filt ? idx->doc_attrs.as<uint2>() : nullptr;
    return OI_OK;
}

// The six arrays of one search's two ranked lists, over either of their two contiguous layouts (L = B * depth); in both the
// BM25 counts follow the cosine counts.
struct SearchLists {
    float *cos_s;
    uint32_t *cos_d, *cos_c;
    float *bm_s;
    uint32_t *bm_d, *bm_c;
    // [cos scores L | cos docs L | bm25 scores L | bm25 docs L | cos counts B | bm25 counts B]
    static size_t block_bytes(uint32_t B, uint32_t depth) { return (size_t)B * depth * 16 + (size_t)B * 8; }
    static SearchLists block(void *p, uint32_t B, uint32_t depth) {
        const size_t L = (size_t)B * depth;
        float *s = static_cast<float *>(p);
        uint32_t *u = static_cast<uint32_t *>(p);
        return {s, u + L, u + 4 * L, s + 2 * L, u + 3 * L, u + 4 * L + B};
    }
    // the exchange format [scores 2L | docs 2L | counts 2B] (cosine first in each): OI_PACKED_WORDS(B, depth) words
    static size_t packed_bytes(uint32_t B, uint32_t depth) { return (size_t)OI_PACKED_WORDS(B, depth) * 4; }
    static SearchLists packed(uint32_t *p, uint32_t B, uint32_t depth) {
        const size_t L = (size_t)B * depth;
        float *s = reinterpret_cast<float *>(p);
        return {s, p + 2 * L, p + 4 * L, s + L, p + 3 * L, p + 4 * L + B};
    }
    int clear_counts(uint32_t B, hipStream_t st) const {
        OI_HIP_CHECK(hipMemsetAsync(cos_c, 0, (size_t)B * 8, st));
        return OI_OK;
    }
    int run(oi_index *idx, const SearchCall &c, uint32_t B, uint32_t depth) const {
        return search_lists_device(idx, c.q.qv, c.q.qt, c.q.qo, B, depth, cos_s, cos_d, cos_c, bm_s, bm_d, bm_c, c.q.filt, c.attrs);
    }
};

// The graph key of a captured search call (location == OI_DEVICE: c.q holds the caller's own pointers).  Words 0-6: the index,
// the call kind with the filters pointer folded in (a filtered call differs from the unfiltered one by it), the query
// pointers, B | depth, the first output pointer.  Word 7: every context / index setting that changes what the call launches --
// add a new one HERE -- under the caller's w7_high; words 8 and 9 are the caller's.
struct SearchKey { uint64_t w[10]; };
SearchKey search_graph_key(oi_index *idx, const SearchCall &c, uint64_t kind, uint32_t B, uint32_t depth, const void *out0,
                           uint32_t w7_high, uint64_t w8, uint64_t w9) {
    const uint64_t mode = ((uint64_t)c.ctx->cosine_mode << 16) | ((uint64_t)idx->bm25_mode << 8) | (c.ctx->overlap_legs ? 1u : 0u);
    return {{idx->uid, kind | ((uint64_t)(uintptr_t)c.q.filt << 8), (uint64_t)(uintptr_t)c.q.qv, (uint64_t)(uintptr_t)c.q.qt,
             (uint64_t)(uintptr_t)c.q.qo, ((uint64_t)B << 32) | depth, (uint64_t)(uintptr_t)out0, ((uint64_t)w7_high << 32) | mode, w8, w9}};
}

// A result block in HBM to the caller's host arrays (null ones skipped): one DMA into the context's page-locked buffer, the
// stream synchronised, host copies.
int results_to_host(oi_ctx *ctx, const ResultBlock &r, float *scores_out, uint32_t *docs_out, uint32_t *counts_out,
                    uint32_t *dup_out = nullptr) {
    OI_CHECK(ctx->pin_out.ensure(r.bytes()));
    OI_HIP_CHECK(hipMemcpyAsync(ctx->pin_out.p, r.scores, r.bytes(), hipMemcpyDeviceToHost, ctx->stream));
    OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    r.at(ctx->pin_out.p).to_arrays(scores_out, docs_out, counts_out, dup_out);
    return OI_OK;
}
// ... the same straight into the caller's arrays, three DMAs and a synchronise (oi_rrf_fuse, oi_merge_lists, oi_fuse_packed:
// calls that make no overflow check)
int results_to_host_direct(oi_ctx *ctx, const ResultBlock &r, float *scores_out, uint32_t *docs_out, uint32_t *counts_out) {
    OI_HIP_CHECK(hipMemcpyAsync(scores_out, r.scores, r.K * 4, hipMemcpyDeviceToHost, ctx->stream));
    OI_HIP_CHECK(hipMemcpyAsync(docs_out, r.docs, r.K * 4, hipMemcpyDeviceToHost, ctx->stream));
    OI_HIP_CHECK(hipMemcpyAsync(counts_out, r.counts, (size_t)r.B * 4, hipMemcpyDeviceToHost, ctx->stream));
    OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return OI_OK;
}

} // namespace

static int search_lists_impl(oi_index *idx, const float *qv, const uint32_t *qt, const uint32_t *qo, uint32_t B,
                             uint32_t depth, int location, float *cos_s, uint32_t *cos_d, uint32_t *cos_c,
                             float *bm_s, uint32_t *bm_d, uint32_t *bm_c, const oi_doc_filter *filters) {
    OI_CHECK(check_search_args(idx, qv, qo, B, depth));
    OI_REQUIRE(cos_s && cos_d && cos_c && bm_s && bm_d && bm_c, "search_lists: null output buffer");
    SearchCall c;
    OI_CHECK(open_search(c, idx, qv, qt, qo, B, location, filters));
    const SearchLists out{cos_s, cos_d, cos_c, bm_s, bm_d, bm_c};
    if (location == OI_DEVICE) return out.run(idx, c, B, depth);
    hipStream_t st = c.ctx->stream;
    const size_t L = (size_t)B * depth, bytes = SearchLists::block_bytes(B, depth);
    DevBuf &o = c.ctx->buf("lists_out");
    OI_CHECK(o.ensure(bytes + 64));
    const SearchLists d = SearchLists::block(o.p, B, depth);
    OI_HIP_CHECK(hipMemsetAsync(o.p, 0, bytes, st));
    OI_CHECK(d.run(idx, c, B, depth));
    OI_HIP_CHECK(hipMemcpyAsync(out.cos_s, d.cos_s, L * 4, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipMemcpyAsync(out.cos_d, d.cos_d, L * 4, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipMemcpyAsync(out.bm_s, d.bm_s, L * 4, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipMemcpyAsync(out.bm_d, d.bm_d, L * 4, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipMemcpyAsync(out.cos_c, d.cos_c, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipMemcpyAsync(out.bm_c, d.bm_c, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipStreamSynchronize(st));
    return check_overflow_locked(c.ctx);
}
extern "C" int oi_search_lists(oi_index *idx, const float *qv, const uint32_t *qt, const uint32_t *qo, uint32_t B,
                               uint32_t depth, int location, float *cos_s, uint32_t *cos_d, uint32_t *cos_c,
                               float *bm_s, uint32_t *bm_d, uint32_t *bm_c) {
    return search_lists_impl(idx, qv, qt, qo, B, depth, location, cos_s, cos_d, cos_c, bm_s, bm_d, bm_c, nullptr);
}
extern "C" int oi_search_lists_filtered(oi_index *idx, const float *qv, const uint32_t *qt, const uint32_t *qo, uint32_t B,
                                        uint32_t depth, const oi_doc_filter *filters, int location, float *cos_s, uint32_t *cos_d,
                                        uint32_t *cos_c, float *bm_s, uint32_t *bm_d, uint32_t *bm_c) {
    return search_lists_impl(idx, qv, qt, qo, B, depth, location, cos_s, cos_d, cos_c, bm_s, bm_d, bm_c, filters);
}

extern "C" int oi_rrf_fuse(oi_ctx *ctx, const uint32_t *docs_a, const uint32_t *counts_a, const uint32_t *docs_b,
                           const uint32_t *counts_b, uint32_t B, uint32_t depth, uint32_t k, int location,
                           float *scores_out, uint32_t *docs_out, uint32_t *counts_out) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(docs_a && counts_a && docs_b && counts_b && scores_out && docs_out && counts_out, "rrf: null buffer");
    if (B == 0) return OI_OK;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    if (location == OI_DEVICE)
        return oi_launch_rrf(ctx, docs_a, counts_a, docs_b, counts_b, B, depth, k, scores_out, docs_out, counts_out);
    hipStream_t st = ctx->stream;
    const size_t L = (size_t)B * depth;
    DevBuf &w = ctx->buf("rrf_io");
    OI_CHECK(w.ensure((2 * L + 2 * (size_t)B) * 4 + ResultBlock::bytes(B, k) + 64));
    uint32_t *d_a = w.as<uint32_t>(), *d_b = d_a + L, *d_ca = d_b + L, *d_cb = d_ca + B;
    const ResultBlock r(d_cb + B, B, k);
    OI_HIP_CHECK(hipMemcpyAsync(d_a, docs_a, L * 4, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemcpyAsync(d_b, docs_b, L * 4, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemcpyAsync(d_ca, counts_a, (size_t)B * 4, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemcpyAsync(d_cb, counts_b, (size_t)B * 4, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemsetAsync(r.scores, 0, r.bytes(), st));
    OI_CHECK(oi_launch_rrf(ctx, d_a, d_ca, d_b, d_cb, B, depth, k, r.scores, r.docs, r.counts));
    return results_to_host_direct(ctx, r, scores_out, docs_out, counts_out);
}

extern "C" int oi_merge_lists(oi_ctx *ctx, const float *scores, const uint32_t *docs, const uint32_t *counts,
                              uint32_t n_shards, uint32_t B, uint32_t depth, int location, float *scores_out,
                              uint32_t *docs_out, uint32_t *counts_out) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(scores && docs && counts && scores_out && docs_out && counts_out, "merge: null buffer");
    OI_REQUIRE(n_shards >= 1 && n_shards <= 1024, "merge: n_shards=%u outside [1,1024]", n_shards);
    OI_REQUIRE(depth >= 1 && depth <= OI_MAX_DEPTH, "merge: depth=%u outside [1,%u]", depth, OI_MAX_DEPTH);
    if (B == 0) return OI_OK;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t carry_cap = OI_MAX_DEPTH;
    const uint64_t mstride = (uint64_t)carry_cap + (uint64_t)n_shards * depth;
    DevBuf &flag = ctx->buf("state_flag");
    if (!flag.p) {
        OI_CHECK(flag.ensure(16));
        OI_HIP_CHECK(hipMemsetAsync(flag.p, 0, 16, st));
    }
    DevBuf &pk = ctx->buf("merge_pool"), &pc = ctx->buf("merge_counts");
    OI_CHECK(pk.ensure(sizeof(uint64_t) * (size_t)B * mstride));
    OI_CHECK(pc.ensure(sizeof(uint32_t) * (size_t)B * (1 + n_shards)));
    PoolView pool{pk.as<uint64_t>(), pc.as<uint32_t>(), pc.as<uint32_t>() + B, nullptr, mstride, carry_cap,
                  depth, n_shards, n_shards, flag.as<uint32_t>()};
    const size_t Lin = (size_t)n_shards * B * depth, Cin = (size_t)n_shards * B;
    if (location == OI_DEVICE) {
        OI_CHECK(oi_launch_lists_to_pool(ctx, scores, docs, counts, (uint64_t)B * depth, B, n_shards, B, depth, pool));
        return oi_launch_select(ctx, pool, B, depth, false, scores_out, docs_out, counts_out, depth);
    }
    DevBuf &w = ctx->buf("merge_io");
    OI_CHECK(w.ensure((2 * Lin + Cin) * 4 + ResultBlock::bytes(B, depth) + 64));
    float *d_s = w.as<float>();
    uint32_t *d_d = reinterpret_cast<uint32_t *>(d_s + Lin), *d_c = d_d + Lin;
    const ResultBlock r(d_c + Cin, B, depth);
    OI_HIP_CHECK(hipMemcpyAsync(d_s, scores, Lin * 4, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemcpyAsync(d_d, docs, Lin * 4, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemcpyAsync(d_c, counts, Cin * 4, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemsetAsync(r.scores, 0, r.bytes(), st));
    OI_CHECK(oi_launch_lists_to_pool(ctx, d_s, d_d, d_c, (uint64_t)B * depth, B, n_shards, B, depth, pool));
    OI_CHECK(oi_launch_select(ctx, pool, B, depth, false, r.scores, r.docs, r.counts, depth));
    return results_to_host_direct(ctx, r, scores_out, docs_out, counts_out);
}

static int search_impl(oi_index *idx, const float *qv, const uint32_t *qt, const uint32_t *qo, uint32_t B,
                       uint32_t depth, uint32_t k, int location, float *scores_out, uint32_t *docs_out,
                       uint32_t *counts_out, const oi_doc_filter *filters) {
    OI_CHECK(check_search_args(idx, qv, qo, B, depth));
    OI_REQUIRE(k >= 1 && k <= OI_MAX_DEPTH, "search: k=%u outside [1,%u]", k, OI_MAX_DEPTH);
    OI_REQUIRE(scores_out && docs_out && counts_out, "search: null output buffer");
    SearchCall c;
    OI_CHECK(open_search(c, idx, qv, qt, qo, B, location, filters));
    oi_ctx *ctx = c.ctx;
    DevBuf &o = ctx->buf("search_lists");
    OI_CHECK(o.ensure(SearchLists::block_bytes(B, depth) + 64));
    const SearchLists l = SearchLists::block(o.p, B, depth);
    auto lists = [&]() -> int {
        OI_CHECK(l.clear_counts(B, ctx->stream));
        return l.run(idx, c, B, depth);
    };
    if (location == OI_DEVICE) {
        const SearchKey key = search_graph_key(idx, c, 3, B, depth, scores_out, 0, ((uint64_t)idx->max_query_terms << 32) | k,
                                               (uint64_t)(uintptr_t)docs_out ^ ((uint64_t)(uintptr_t)counts_out << 1));
        return run_captured(ctx, key.w, [&]() -> int {
            OI_CHECK(lists());
            return oi_launch_rrf(ctx, l.cos_d, l.cos_c, l.bm_d, l.bm_c, B, depth, k, scores_out, docs_out, counts_out);
        });
    }
    OI_CHECK(lists());
    DevBuf &f = ctx->buf("search_out");
    OI_CHECK(f.ensure(ResultBlock::bytes(B, k) + 64));
    const ResultBlock r(f.p, B, k);
    OI_HIP_CHECK(hipMemsetAsync(f.p, 0, r.bytes(), ctx->stream));
    OI_CHECK(oi_launch_rrf(ctx, l.cos_d, l.cos_c, l.bm_d, l.bm_c, B, depth, k, r.scores, r.docs, r.counts));
    OI_CHECK(results_to_host(ctx, r, scores_out, docs_out, counts_out));
    return check_overflow_locked(ctx);
}
extern "C" int oi_search(oi_index *idx, const float *qv, const uint32_t *qt, const uint32_t *qo, uint32_t B,
                         uint32_t depth, uint32_t k, int location, float *scores_out, uint32_t *docs_out,
                         uint32_t *counts_out) {
    return search_impl(idx, qv, qt, qo, B, depth, k, location, scores_out, docs_out, counts_out, nullptr);
}
extern "C" int oi_search_filtered(oi_index *idx, const float *qv, const uint32_t *qt, const uint32_t *qo, uint32_t B,
                                  uint32_t depth, uint32_t k, const oi_doc_filter *filters, int location, float *scores_out,
                                  uint32_t *docs_out, uint32_t *counts_out) {
    return search_impl(idx, qv, qt, qo, B, depth, k, location, scores_out, docs_out, counts_out, filters);
}

// ---------------------------------------------------------------- near-duplicate collapse (collapse.hip)
// Every argument check precedes the first HIP call (the scalars first: they can be judged without a handle).
static int check_collapse_args(const char *what, float threshold, uint32_t depth, uint32_t k) {
    OI_REQUIRE(threshold == threshold, "%s: threshold is NaN", what);
    OI_REQUIRE(depth >= 1 && depth <= OI_MAX_DEPTH, "%s: depth / pool = %u outside [1,%u]", what, depth, OI_MAX_DEPTH);
    OI_REQUIRE(k >= 1 && k <= OI_MAX_DEPTH, "%s: k=%u outside [1,%u]", what, k, OI_MAX_DEPTH);
    return OI_OK;
}
static int check_collapse_state(const char *what, oi_index *idx) {
    if (!idx) { oi_set_error("%s: null index", what); return OI_ERR_INVALID_ARG; }
    if (!idx->rows && !idx->rows_bf16) { oi_set_error("%s: the index has no embeddings (oi_index_set_embeddings)", what); return OI_ERR_STATE; }
    return OI_OK;
}
extern "C" int oi_collapse_lists(oi_index *idx, const float *scores, const uint32_t *docs, const uint32_t *counts, uint32_t B,
                                 uint32_t depth, float threshold, uint32_t k, int location, float *scores_out, uint32_t *docs_out,
                                 uint32_t *counts_out, uint32_t *dup_counts_out) {
    OI_CHECK(check_collapse_args("collapse_lists", threshold, depth, k));
    OI_REQUIRE(docs && counts && docs_out && counts_out, "collapse_lists: null buffer");
    OI_REQUIRE(!scores || scores_out, "collapse_lists: scores given without scores_out");
    OI_CHECK(check_collapse_state("collapse_lists", idx));
    if (B == 0) return OI_OK;
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    if (!scores) scores_out = nullptr;
    if (location == OI_DEVICE)
        return oi_launch_collapse(idx, scores, docs, counts, B, depth, threshold, k, scores_out, docs_out, counts_out, dup_counts_out);
    hipStream_t st = ctx->stream;
    const size_t L = (size_t)B * depth;
    DevBuf &w = ctx->buf("collapse_io");
    OI_CHECK(w.ensure((2 * L + B) * 4 + ResultBlock::bytes(B, k, true) + 64));
    uint32_t *d_d = w.as<uint32_t>(), *d_c = d_d + L;
    float *d_s = reinterpret_cast<float *>(d_c + B);
    const ResultBlock r(d_s + L, B, k, true);
    OI_HIP_CHECK(hipMemcpyAsync(d_d, docs, L * 4, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemcpyAsync(d_c, counts, (size_t)B * 4, hipMemcpyHostToDevice, st));
    if (scores) OI_HIP_CHECK(hipMemcpyAsync(d_s, scores, L * 4, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemsetAsync(r.scores, 0, r.bytes(), st));
    OI_CHECK(oi_launch_collapse(idx, scores ? d_s : nullptr, d_d, d_c, B, depth, threshold, k, scores ? r.scores : nullptr, r.docs, r.counts, r.dup));
    return results_to_host(ctx, r, scores_out, docs_out, counts_out, dup_counts_out);
}

// oi_search_filtered(depth, k = pool) into a device buffer, then the collapse of that fused list
extern "C" int oi_search_collapsed(oi_index *idx, const float *qv, const uint32_t *qt, const uint32_t *qo, uint32_t B, uint32_t depth,
                                   uint32_t pool, uint32_t k, float threshold, const oi_doc_filter *filters, int location,
                                   float *scores_out, uint32_t *docs_out, uint32_t *counts_out, uint32_t *dup_counts_out) {
    OI_CHECK(check_collapse_args("search_collapsed", threshold, pool, k));
    OI_REQUIRE(k <= pool, "search_collapsed: k=%u exceeds pool=%u", k, pool);
    OI_REQUIRE(scores_out && docs_out && counts_out, "search_collapsed: null output buffer");
    OI_CHECK(check_collapse_state("search_collapsed", idx));
    OI_CHECK(check_search_args(idx, qv, qo, B, depth));
    SearchCall c;
    OI_CHECK(open_search(c, idx, qv, qt, qo, B, location, filters));
    oi_ctx *ctx = c.ctx;
    DevBuf &o = ctx->buf("search_lists"), &pl = ctx->buf("collapse_pool");
    OI_CHECK(o.ensure(SearchLists::block_bytes(B, depth) + 64));
    OI_CHECK(pl.ensure(ResultBlock::bytes(B, pool) + 64));
    const SearchLists l = SearchLists::block(o.p, B, depth);
    const ResultBlock fused(pl.p, B, pool); // the fused pool-list: it never leaves the device
    auto body = [&](float *so, uint32_t *dd, uint32_t *co, uint32_t *dup) -> int {
        OI_CHECK(l.clear_counts(B, ctx->stream));
        OI_CHECK(l.run(idx, c, B, depth));
        OI_CHECK(oi_launch_rrf(ctx, l.cos_d, l.cos_c, l.bm_d, l.bm_c, B, depth, pool, fused.scores, fused.docs, fused.counts));
        return oi_launch_collapse(idx, fused.scores, fused.docs, fused.counts, B, pool, threshold, k, so, dd, co, dup);
    };
    if (location == OI_DEVICE) {
        uint32_t tbits;
        memcpy(&tbits, &threshold, 4);
        const SearchKey key = search_graph_key(
            idx, c, 5, B, depth, scores_out, tbits, ((uint64_t)idx->max_query_terms << 32) | ((uint64_t)pool << 16) | k,
            (uint64_t)(uintptr_t)docs_out ^ ((uint64_t)(uintptr_t)counts_out << 1) ^ ((uint64_t)(uintptr_t)dup_counts_out << 2));
        return run_captured(ctx, key.w, [&]() -> int { return body(scores_out, docs_out, counts_out, dup_counts_out); });
    }
    DevBuf &f = ctx->buf("collapse_out");
    OI_CHECK(f.ensure(ResultBlock::bytes(B, k, true) + 64));
    const ResultBlock r(f.p, B, k, true);
    OI_HIP_CHECK(hipMemsetAsync(f.p, 0, r.bytes(), ctx->stream));
    OI_CHECK(body(r.scores, r.docs, r.counts, r.dup));
    OI_CHECK(results_to_host(ctx, r, scores_out, docs_out, counts_out, dup_counts_out));
    return check_overflow_locked(ctx);
}

// ---------------------------------------------------------------- the analytics family's entry points
// The threshold family (oi_volume.h), the mention summary (mention.hip), narrative discovery (centroids.hip, 4.14),
// its seeding (seeds.hip, 4.16), narrative terms (label_terms.hip, 4.17), exemplars (label_exemplars.hip, 4.18) and the
// breakdown (label_summary.hip, 4.19).  What they check and stage alike is written once; `call` is the entry point's name in
// the messages.
// The family's order of checks: the spec first (it can be judged without a handle), the numbers, the buffers, the location
// (in the calls that check it), then the handle and its state, which takes the context's lock; all of them precede the first
// HIP call.  OI_DEVICE: oi_label_terms, oi_label_exemplars and oi_label_summary make no host synchronise anywhere.  None of
// the calls is ever captured.

// One axis of cells.  The key axis: `mask` is one contiguous run of bits, there is no bucket width, n_cells lies within the key
// space.  The time axis: the bucket rules (mask is not looked at).  cells_name: what the call's spec calls n_cells.
static int check_axis(const char *call, bool key_axis, uint32_t mask, uint32_t bucket_width, uint32_t n_cells, const char *cells_name) {
    if (key_axis) {
        const uint32_t run = mask ? mask >> __builtin_ctz(mask) : 0u;
        OI_REQUIRE(mask != 0 && (run & (run + 1u)) == 0u, "%s: key_mask=0x%x is not one contiguous run of bits", call, mask);
        OI_REQUIRE(bucket_width == 0, "%s: bucket_width=%u on the key axis (must be 0)", call, bucket_width);
        const uint64_t key_space = std::min<uint64_t>(1ull << __builtin_popcount(mask), OI_MAX_GROUP_KEYS);
        OI_REQUIRE(n_cells >= 1 && n_cells <= key_space, "%s: %s=%u outside [1,%llu] (key_mask=0x%x)", call, cells_name, n_cells,
                   (unsigned long long)key_space, mask);
        return OI_OK;
    }
    OI_REQUIRE(n_cells >= 1 && n_cells <= OI_MAX_VOLUME_BUCKETS, "%s: %s=%u outside [1,%u]", call, cells_name, n_cells, OI_MAX_VOLUME_BUCKETS);
    OI_REQUIRE(bucket_width != 0 || n_cells == 1, "%s: bucket_width=0 (no time axis) with %s=%u", call, cells_name, n_cells);
    return OI_OK;
}
static int check_clusters(const char *call, uint32_t K) {
    OI_REQUIRE(K >= 1 && K <= OI_MAX_CENTROIDS, "%s: n_clusters=%u outside [1,%u]", call, K, OI_MAX_CENTROIDS);
    return OI_OK;
}
static int check_location(const char *call, int location) {
    OI_REQUIRE(location == OI_HOST || location == OI_DEVICE, "%s: bad location %d", call, location);
    return OI_OK;
}
// every_list: the postings buffer must exist even where the index holds no posting (the mention summary's rule)
static int check_finalized(const char *call, const oi_index *idx, bool every_list) {
    if (!idx->finalized || !idx->cell_start.p || ((every_list || idx->n_postings) && !idx->postings.p)) {
        oi_set_error("%s: the index is not finalized (oi_index_finalize makes the postings)", call);
        return OI_ERR_STATE;
    }
    return OI_OK;
}

// The spec of the calls with a threshold and a time axis.  per_query: the call takes a thresholds array; max_cells: its cap on
// n_queries * n_buckets (0: none).
static int similar_check_spec(const char *call, float threshold, const float *thresholds, bool per_query, uint32_t n_buckets,
                              uint32_t bucket_width, uint32_t B, uint32_t max_cells) {
    OI_REQUIRE(thresholds || threshold == threshold, "%s: threshold is NaN%s", call, per_query ? " (and no thresholds array)" : "");
    OI_CHECK(check_axis(call, false, 0, bucket_width, n_buckets, "n_buckets"));
    OI_REQUIRE(B <= 4096, "%s: n_queries=%u outside [0,4096]", call, B);
    OI_REQUIRE(!max_cells || (uint64_t)B * n_buckets <= max_cells, "%s: n_queries * n_buckets = %llu cells, more than %u", call,
               (unsigned long long)B * n_buckets, max_cells);
    return OI_OK;
}

// The index and what of its state the call needs.  g takes the context's lock where every call took it: behind the embeddings
// check.  attrs_for: who needs the doc attributes ("... need" / "... needs"), or null when this call does not.
enum : unsigned { NEED_ROWS = 1, NEED_SIGNALS = 2, NEED_POSTINGS = 4 };
static int check_index_state(const char *call, oi_index *idx, unsigned needs, const char *attrs_for, std::unique_lock<std::mutex> &g) {
    if (!idx) { oi_set_error("%s: null index", call); return OI_ERR_INVALID_ARG; }
    if ((needs & NEED_ROWS) && !idx->rows && !idx->rows_bf16) { oi_set_error("%s: the index has no embeddings (oi_index_set_embeddings)", call); return OI_ERR_STATE; }
    g = std::unique_lock<std::mutex>(idx->ctx->mu);
    if (needs & NEED_POSTINGS) OI_CHECK(check_finalized(call, idx, true));
    if ((needs & NEED_SIGNALS) && !idx->signals.p) { oi_set_error("%s: the index has no signals (oi_index_set_signals)", call); return OI_ERR_STATE; }
    if (attrs_for && !idx->doc_attrs.p) {
        oi_set_error("%s: %s the index's doc attributes (oi_index_set_doc_attrs)", call, attrs_for);
        return OI_ERR_STATE;
    }
    return OI_OK;
}
#define SIMILAR_TIME_AXIS "filters / time buckets need"

// The host location of every call of the family: [inputs ... | outputs ...] in the call's workspace `io`, each part aligned to
// `granule`.  The inputs are copied in; launch(in, out) gets the parts' device pointers; then every output with a host pointer
// is copied back and the stream awaited.  An input without a host pointer is absent: no room, in[i] null.  An output of 0 bytes
// is absent: out[i] null; one without a host pointer still has its room, the launch may write it.
struct StageIn { const void *host; size_t bytes; };
struct StageOut { void *host; size_t bytes; };
template <size_t NI, size_t NO, class Launch>
static int staged_call(oi_ctx *ctx, const char *io, size_t granule, const StageIn (&ins)[NI], const StageOut (&outs)[NO], Launch launch) {
    static_assert(sizeof(oi_doc_filter) == sizeof(uint4), "oi_doc_filter is 16 bytes");
    hipStream_t st = ctx->stream;
    StageLayout lay(granule);
    size_t in_at[NI], out_at[NO];
    for (size_t i = 0; i < NI; ++i) in_at[i] = lay.add(ins[i].host ? ins[i].bytes : 0);
    for (size_t i = 0; i < NO; ++i) out_at[i] = lay.add(outs[i].bytes);
    DevBuf &w = ctx->buf(io);
    OI_CHECK(w.ensure(lay.total()));
    void *in[NI], *out[NO];
    for (size_t i = 0; i < NI; ++i) {
        in[i] = ins[i].host ? lay.at<void>(w.p, in_at[i]) : nullptr;
        if (ins[i].host && ins[i].bytes) OI_HIP_CHECK(hipMemcpyAsync(in[i], ins[i].host, ins[i].bytes, hipMemcpyHostToDevice, st));
    }
    for (size_t i = 0; i < NO; ++i) out[i] = outs[i].bytes ? lay.at<void>(w.p, out_at[i]) : nullptr;
    OI_CHECK(launch(in, out));
    for (size_t i = 0; i < NO; ++i)
        if (outs[i].host && outs[i].bytes) OI_HIP_CHECK(hipMemcpyAsync(outs[i].host, out[i], outs[i].bytes, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipStreamSynchronize(st));
    return OI_OK;
}
template <class T> static T *part(void *const *parts, size_t i) { return static_cast<T *>(parts[i]); }
// the staged inputs of the threshold family: the query vectors, the filters, the thresholds (the last two may be null)
#define SIMILAR_INPUTS(thresholds) \
    {{qv, sizeof(float) * (size_t)B * idx->dim}, {filters, sizeof(oi_doc_filter) * (size_t)B}, {thresholds, sizeof(float) * (size_t)B}}

// similarity volume (cosine_volume.hip)
extern "C" int oi_similar_volume(oi_index *idx, const float *qv, uint32_t B, const oi_volume_spec *spec, const oi_doc_filter *filters,
                                 int location, uint32_t *counts_out) {
    OI_REQUIRE(spec, "similar_volume: null spec");
    OI_CHECK(similar_check_spec("similar_volume", spec->threshold, nullptr, false, spec->n_buckets, spec->bucket_width, B, 0));
    OI_REQUIRE(B == 0 || (qv && counts_out), "similar_volume: null buffer");
    std::unique_lock<std::mutex> g;
    OI_CHECK(check_index_state("similar_volume", idx, NEED_ROWS, (filters || spec->bucket_width) ? SIMILAR_TIME_AXIS : nullptr, g));
    if (B == 0) return OI_OK;
    OI_HIP_CHECK(hipSetDevice(idx->ctx->device));
    if (location == OI_DEVICE) return oi_launch_similar_volume(idx, qv, B, *spec, reinterpret_cast<const uint4 *>(filters), counts_out);
    return staged_call(idx->ctx, "volume_io", 16, SIMILAR_INPUTS(nullptr), {{counts_out, sizeof(uint32_t) * (size_t)B * spec->n_buckets}},
                       [&](void *const *in, void *const *out) {
                           return oi_launch_similar_volume(idx, part<const float>(in, 0), B, *spec, part<const uint4>(in, 1), part<uint32_t>(out, 0));
                       });
}

// similarity summary (cosine_summary.hip)
extern "C" int oi_similar_summary(oi_index *idx, const float *qv, uint32_t B, const oi_summary_spec *spec, const float *thresholds,
                                  const oi_doc_filter *filters, int location, oi_social_counters *out) {
    OI_REQUIRE(spec, "similar_summary: null spec");
    OI_CHECK(similar_check_spec("similar_summary", spec->threshold, thresholds, true, spec->n_buckets, spec->bucket_width, B, OI_MAX_SUMMARY_CELLS));
    OI_REQUIRE(B == 0 || (qv && out), "similar_summary: null buffer");
    std::unique_lock<std::mutex> g;
    OI_CHECK(check_index_state("similar_summary", idx, NEED_ROWS | NEED_SIGNALS, (filters || spec->bucket_width) ? SIMILAR_TIME_AXIS : nullptr, g));
    if (B == 0) return OI_OK;
    OI_HIP_CHECK(hipSetDevice(idx->ctx->device));
    if (location == OI_DEVICE)
        return oi_launch_similar_summary(idx, qv, B, *spec, thresholds, reinterpret_cast<const uint4 *>(filters), out);
    return staged_call(idx->ctx, "summary_io", 16, SIMILAR_INPUTS(thresholds), {{out, sizeof(oi_social_counters) * (size_t)B * spec->n_buckets}},
                       [&](void *const *in, void *const *o) {
                           return oi_launch_similar_summary(idx, part<const float>(in, 0), B, *spec, part<const float>(in, 2), part<const uint4>(in, 1),
                                                            part<oi_social_counters>(o, 0));
                       });
}

// similarity leaderboard (cosine_groups.hip): its spec is its own, the rest as above
extern "C" int oi_similar_groups(oi_index *idx, const float *qv, uint32_t B, const oi_groups_spec *spec, const float *thresholds,
                                 const oi_doc_filter *filters, int location, oi_social_counters *records_out, uint32_t *keys_out,
                                 uint32_t *counts_out, uint32_t *qualified_out) {
    OI_REQUIRE(spec, "similar_groups: null spec");
    OI_REQUIRE(thresholds || spec->threshold == spec->threshold, "similar_groups: threshold is NaN (and no thresholds array)");
    OI_CHECK(check_axis("similar_groups", true, spec->key_mask, 0, spec->n_keys, "n_keys"));
    OI_REQUIRE(spec->top <= OI_MAX_DEPTH, "similar_groups: top=%u outside [0,%u]", spec->top, OI_MAX_DEPTH);
    OI_REQUIRE(spec->rank_by <= OI_GROUP_RANK_BEARISH, "similar_groups: rank_by=%u is not an OI_GROUP_RANK_* value", spec->rank_by);
    OI_REQUIRE(B <= 4096, "similar_groups: n_queries=%u outside [0,4096]", B);
    OI_REQUIRE((uint64_t)B * spec->n_keys <= OI_MAX_GROUP_CELLS, "similar_groups: n_queries * n_keys = %llu cells, more than %u",
               (unsigned long long)B * spec->n_keys, OI_MAX_GROUP_CELLS);
    OI_REQUIRE(B == 0 || (qv && records_out), "similar_groups: null buffer");
    OI_REQUIRE(B == 0 || spec->top == 0 || (keys_out && counts_out), "similar_groups: null buffer (keys_out / counts_out with top=%u)", spec->top);
    std::unique_lock<std::mutex> g;
    OI_CHECK(check_index_state("similar_groups", idx, NEED_ROWS | NEED_SIGNALS, "the key axis needs", g));
    if (B == 0) return OI_OK;
    OI_HIP_CHECK(hipSetDevice(idx->ctx->device));
    if (location == OI_DEVICE)
        return oi_launch_similar_groups(idx, qv, B, *spec, thresholds, reinterpret_cast<const uint4 *>(filters), records_out, keys_out,
                                        counts_out, qualified_out);
    const size_t per_q = spec->top ? spec->top : spec->n_keys; // records (and, ranked, keys) per query
    const size_t kb = spec->top ? sizeof(uint32_t) * (size_t)B * per_q : 0, cb = spec->top ? sizeof(uint32_t) * (size_t)B : 0;
    return staged_call(idx->ctx, "groups_io", 16, SIMILAR_INPUTS(thresholds),
                       {{records_out, sizeof(oi_social_counters) * (size_t)B * per_q}, {keys_out, kb}, {counts_out, cb}, {qualified_out, cb}},
                       [&](void *const *in, void *const *out) { // (dense: keys, counts and qualified are absent)
                           return oi_launch_similar_groups(idx, part<const float>(in, 0), B, *spec, part<const float>(in, 2), part<const uint4>(in, 1),
                                                           part<oi_social_counters>(out, 0), part<uint32_t>(out, 1), part<uint32_t>(out, 2),
                                                           part<uint32_t>(out, 3));
                       });
}

// similarity share (cosine_share.hip).  labels_out may be null.
extern "C" int oi_similar_share(oi_index *idx, const float *qv, uint32_t B, const oi_summary_spec *spec, const float *thresholds,
                                const oi_doc_filter *filters, int location, oi_social_counters *out, uint32_t *labels_out) {
    OI_REQUIRE(spec, "similar_share: null spec");
    OI_CHECK(similar_check_spec("similar_share", spec->threshold, thresholds, true, spec->n_buckets, spec->bucket_width, B, OI_MAX_SUMMARY_CELLS));
    OI_REQUIRE(B == 0 || (qv && out), "similar_share: null buffer");
    std::unique_lock<std::mutex> g;
    OI_CHECK(check_index_state("similar_share", idx, NEED_ROWS | NEED_SIGNALS, (filters || spec->bucket_width) ? SIMILAR_TIME_AXIS : nullptr, g));
    OI_HIP_CHECK(hipSetDevice(idx->ctx->device));
    const size_t lb = labels_out ? sizeof(uint32_t) * (size_t)idx->n_docs : 0;
    if (B == 0) { // no query: no row has a candidate
        if (lb && location == OI_DEVICE) OI_HIP_CHECK(hipMemsetAsync(labels_out, 0xFF, lb, idx->ctx->stream));
        else if (lb) memset(labels_out, 0xFF, lb);
        return OI_OK;
    }
    if (location == OI_DEVICE)
        return oi_launch_similar_share(idx, qv, B, *spec, thresholds, reinterpret_cast<const uint4 *>(filters), out, labels_out);
    return staged_call(idx->ctx, "share_io", 16, SIMILAR_INPUTS(thresholds),
                       {{out, sizeof(oi_social_counters) * (size_t)B * spec->n_buckets}, {labels_out, lb}}, [&](void *const *in, void *const *o) {
                           return oi_launch_similar_share(idx, part<const float>(in, 0), B, *spec, part<const float>(in, 2), part<const uint4>(in, 1),
                                                          part<oi_social_counters>(o, 0), part<uint32_t>(o, 1));
                       });
}

// mention summary (mention.hip)
extern "C" int oi_mention_summary(oi_index *idx, const uint32_t *qt, const uint32_t *qo, uint32_t B, const oi_mention_spec *spec,
                                  const uint32_t *min_match, const oi_doc_filter *filters, int location, oi_social_counters *out) {
    OI_REQUIRE(spec, "mention_summary: null spec");
    OI_REQUIRE(spec->axis == OI_MENTION_AXIS_TIME || spec->axis == OI_MENTION_AXIS_KEY, "mention_summary: axis=%u is not an OI_MENTION_AXIS_* value",
               spec->axis);
    const bool key_axis = spec->axis == OI_MENTION_AXIS_KEY;
    OI_CHECK(check_axis("mention_summary", key_axis, spec->stamp_origin, spec->bucket_width, spec->n_cells, "n_cells"));
    OI_REQUIRE(B <= 4096, "mention_summary: n_queries=%u outside [0,4096]", B);
    OI_REQUIRE((uint64_t)B * spec->n_cells <= OI_MAX_GROUP_CELLS, "mention_summary: n_queries * n_cells = %llu cells, more than %u",
               (unsigned long long)B * spec->n_cells, OI_MAX_GROUP_CELLS);
    OI_REQUIRE(B == 0 || (qt && qo && out), "mention_summary: null buffer");
    OI_CHECK(check_location("mention_summary", location));
    uint32_t nt = 0;
    if (location == OI_HOST && B) { // (device offsets are not host-visible: the plan kernel refuses such a query by itself)
        for (uint32_t q = 0; q < B; ++q) {
            OI_REQUIRE(qo[q + 1] >= qo[q], "mention_summary: q_term_offsets decrease at query %u", q);
            OI_REQUIRE(qo[q + 1] - qo[q] <= OI_MAX_MENTION_TERMS, "mention_summary: query %u has %u terms, more than %u", q, qo[q + 1] - qo[q],
                       OI_MAX_MENTION_TERMS);
        }
        nt = qo[B] - qo[0];
    }
    std::unique_lock<std::mutex> g;
    OI_CHECK(check_index_state("mention_summary", idx, NEED_SIGNALS | NEED_POSTINGS,
                               key_axis ? "the key axis needs" : (filters || spec->bucket_width) ? SIMILAR_TIME_AXIS : nullptr, g));
    OI_REQUIRE((uint64_t)idx->n_blocks * B <= 0xFFFFFFFFull, "mention_summary: %llu (query, doc block) tasks, more than 2^32 - 1",
               (unsigned long long)idx->n_blocks * B);
    if (B == 0) return OI_OK;
    oi_ctx *ctx = idx->ctx;
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    if (location == OI_DEVICE) return oi_launch_mention_summary(idx, qt, qo, B, *spec, min_match, reinterpret_cast<const uint4 *>(filters), out);
    std::vector<uint32_t> rel(qo, qo + B + 1); // offsets relative to the first staged term
    for (uint32_t &o : rel) o -= qo[0];
    return staged_call(ctx, "mention_io", 16,
                       {{rel.data(), sizeof(uint32_t) * ((size_t)B + 1)}, {qt + qo[0], sizeof(uint32_t) * (size_t)nt},
                        {min_match, sizeof(uint32_t) * (size_t)B}, {filters, sizeof(oi_doc_filter) * (size_t)B}},
                       {{out, sizeof(oi_social_counters) * (size_t)B * spec->n_cells}}, [&](void *const *in, void *const *o) -> int {
                           OI_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (`rel` is pageable and dies with this call)
                           return oi_launch_mention_summary(idx, part<const uint32_t>(in, 1), part<const uint32_t>(in, 0), B, *spec,
                                                            part<const uint32_t>(in, 2), part<const uint4>(in, 3), part<oi_social_counters>(o, 0));
                       });
}

// ---- narrative discovery (centroids.hip)
// the update step's reduction: labels -> integer sums and counts per cluster
extern "C" int oi_label_sums(oi_index *idx, const uint32_t *labels, uint32_t K, int location, int64_t *sums_out, uint64_t *counts_out) {
    OI_CHECK(check_clusters("label_sums", K));
    OI_REQUIRE(labels && sums_out && counts_out, "label_sums: null buffer");
    std::unique_lock<std::mutex> g;
    OI_CHECK(check_index_state("label_sums", idx, NEED_ROWS, nullptr, g));
    OI_HIP_CHECK(hipSetDevice(idx->ctx->device));
    if (location == OI_DEVICE) return oi_launch_label_sums(idx, labels, K, sums_out, counts_out);
    return staged_call(idx->ctx, "label_sums_io", 16, {{labels, sizeof(uint32_t) * (size_t)idx->n_docs}},
                       {{sums_out, sizeof(int64_t) * (size_t)K * idx->dim}, {counts_out, sizeof(uint64_t) * (size_t)K}},
                       [&](void *const *in, void *const *out) {
                           return oi_launch_label_sums(idx, part<const uint32_t>(in, 0), K, part<int64_t>(out, 0), part<uint64_t>(out, 1));
                       });
}

// sums -> unit vectors
extern "C" int oi_centroids_from_sums(oi_ctx *ctx, const int64_t *sums, const uint64_t *counts, const float *previous, uint32_t K,
                                      uint32_t dim, int location, float *out) {
    OI_CHECK(check_clusters("centroids_from_sums", K));
    OI_REQUIRE(dim >= 4 && dim <= OI_MAX_DIM && dim % 4 == 0, "centroids_from_sums: dim=%u is not a multiple of 4 in [4,%u]", dim, OI_MAX_DIM);
    OI_REQUIRE(sums && counts && out, "centroids_from_sums: null buffer");
    OI_REQUIRE(ctx, "centroids_from_sums: null ctx");
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    if (location == OI_DEVICE) return oi_launch_centroids_from_sums(ctx, sums, counts, previous, K, dim, out);
    const size_t vb = sizeof(float) * (size_t)K * dim;
    return staged_call(ctx, "centroids_io", 16, {{sums, sizeof(int64_t) * (size_t)K * dim}, {counts, sizeof(uint64_t) * (size_t)K}}, {{out, vb}},
                       [&](void *const *in, void *const *o) -> int { // (in place: `previous` is staged where the output goes, the aliasing form)
                           float *d_v = part<float>(o, 0);
                           if (previous) OI_HIP_CHECK(hipMemcpyAsync(d_v, previous, vb, hipMemcpyHostToDevice, ctx->stream));
                           return oi_launch_centroids_from_sums(ctx, part<const int64_t>(in, 0), part<const uint64_t>(in, 1), previous ? d_v : nullptr,
                                                                K, dim, d_v);
                       });
}

// the loop: assignment (oi_launch_similar_share) and update alternate on the device; the host reads `moved` once per step
extern "C" int oi_narratives_fit(oi_index *idx, const float *seeds, uint32_t K, const oi_narrative_spec *spec, const oi_doc_filter *filter,
                                 int location, float *centroids_out, oi_social_counters *records_out, uint32_t *labels_out,
                                 oi_narrative_info *info_host) {
    OI_REQUIRE(spec, "narratives_fit: null spec");
    OI_CHECK(check_clusters("narratives_fit", K));
    OI_REQUIRE(spec->max_iters >= 1 && spec->max_iters <= 64, "narratives_fit: max_iters=%u outside [1,64]", spec->max_iters);
    OI_CHECK(similar_check_spec("narratives_fit", spec->threshold, nullptr, false, spec->n_buckets, spec->bucket_width, K, OI_MAX_SUMMARY_CELLS));
    OI_REQUIRE(seeds && centroids_out && records_out && info_host, "narratives_fit: null buffer");
    std::unique_lock<std::mutex> g;
    OI_CHECK(check_index_state("narratives_fit", idx, NEED_ROWS | NEED_SIGNALS, (filter || spec->bucket_width) ? SIMILAR_TIME_AXIS : nullptr, g));
    oi_ctx *ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    const oi_summary_spec ss = {spec->threshold, spec->stamp_origin, spec->bucket_width, spec->n_buckets};
    const uint64_t n = idx->n_docs;
    const uint32_t dim = idx->dim;
    const bool host = location != OI_DEVICE;
    const size_t lb = sizeof(uint32_t) * (size_t)n, vb = sizeof(float) * (size_t)K * dim, rb = sizeof(oi_social_counters) * (size_t)K * spec->n_buckets;
    // the workspace: two label arrays | sums | counts | two centroid sets | the filter, K times | moved | the records (OI_HOST)
    StageLayout lay(256);
    const size_t at_lab[2] = {lay.add(lb), lay.add(lb)}, at_sums = lay.add(sizeof(int64_t) * (size_t)K * dim), at_counts = lay.add(sizeof(uint64_t) * (size_t)K);
    const size_t at_c[2] = {lay.add(vb), lay.add(vb)}, at_filt = lay.add(sizeof(oi_doc_filter) * (size_t)K), at_moved = lay.add(256);
    const size_t at_rec = lay.add(host ? rb : 0);
    DevBuf &w = ctx->buf("narratives");
    OI_CHECK(w.ensure(lay.total()));
    uint32_t *d_lab[2] = {lay.at<uint32_t>(w.p, at_lab[0]), lay.at<uint32_t>(w.p, at_lab[1])};
    int64_t *d_sums = lay.at<int64_t>(w.p, at_sums);
    uint64_t *d_counts = lay.at<uint64_t>(w.p, at_counts), *d_moved = lay.at<uint64_t>(w.p, at_moved);
    float *d_c[2] = {lay.at<float>(w.p, at_c[0]), lay.at<float>(w.p, at_c[1])};
    uint4 *d_filt = lay.at<uint4>(w.p, at_filt);
    oi_social_counters *d_rec = host ? lay.at<oi_social_counters>(w.p, at_rec) : records_out;

    OI_HIP_CHECK(hipMemcpyAsync(d_c[0], seeds, vb, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    if (filter) {
        std::vector<oi_doc_filter> rep(K, *filter);
        OI_HIP_CHECK(hipMemcpyAsync(d_filt, rep.data(), sizeof(oi_doc_filter) * (size_t)K, hipMemcpyHostToDevice, st));
        OI_HIP_CHECK(hipStreamSynchronize(st)); // (rep leaves scope)
    }
    if (n) OI_HIP_CHECK(hipMemsetAsync(d_lab[1], 0xFF, lb, st)); // labels_0: nobody is assigned
    oi_narrative_info info = {0, 0, 0, 0};
    int cur = 0;
    for (uint32_t i = 1;; ++i) {
        uint64_t moved[2] = {0, 0};
        OI_CHECK(oi_launch_similar_share(idx, d_c[cur], K, ss, nullptr, filter ? d_filt : nullptr, d_rec, d_lab[cur]));
        OI_CHECK(oi_launch_fit_moved(ctx, d_lab[cur], d_lab[cur ^ 1], n, d_moved));
        OI_HIP_CHECK(hipMemcpyAsync(moved, d_moved, sizeof(moved), hipMemcpyDeviceToHost, st));
        OI_HIP_CHECK(hipStreamSynchronize(st));
        info.iterations = i;
        info.moved = moved[0];
        info.assigned = moved[1];
        if (i > 1 && moved[0] == 0) { info.converged = 1; break; }
        if (i == spec->max_iters) break;
        OI_CHECK(oi_launch_label_sums(idx, d_lab[cur], K, d_sums, d_counts));
        OI_CHECK(oi_launch_centroids_from_sums(ctx, d_sums, d_counts, d_c[cur], K, dim, d_c[cur ^ 1]));
        cur ^= 1; // (centroid set and label array swap together: d_lab[cur ^ 1] is now the previous step's)
    }
    const hipMemcpyKind out_kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    OI_HIP_CHECK(hipMemcpyAsync(centroids_out, d_c[cur], vb, out_kind, st));
    if (host) OI_HIP_CHECK(hipMemcpyAsync(records_out, d_rec, rb, hipMemcpyDeviceToHost, st));
    if (labels_out && n) OI_HIP_CHECK(hipMemcpyAsync(labels_out, d_lab[cur], lb, out_kind, st));
    OI_HIP_CHECK(hipStreamSynchronize(st));
    *info_host = info;
    return OI_OK;
}

// the seeding (seeds.hip): no host synchronise between the steps; one at the end when the caller reads the info, which comes
// from the launcher's own workspace
extern "C" int oi_narratives_seed(oi_index *idx, uint32_t K, const oi_seed_spec *spec, const oi_doc_filter *filter, int location,
                                  float *seeds_out, uint32_t *rows_out, oi_seed_info *info_host) {
    OI_REQUIRE(spec, "narratives_seed: null spec");
    OI_CHECK(check_clusters("narratives_seed", K));
    OI_REQUIRE(spec->method == OI_SEED_KMEANSPP || spec->method == OI_SEED_FARTHEST, "narratives_seed: method=%u is not an OI_SEED_* value",
               spec->method);
    OI_REQUIRE(spec->trials >= 1 && spec->trials <= OI_MAX_SEED_TRIALS, "narratives_seed: trials=%u outside [1,%u]", spec->trials,
               OI_MAX_SEED_TRIALS);
    OI_REQUIRE(spec->method != OI_SEED_FARTHEST || spec->trials == 1, "narratives_seed: trials=%u with OI_SEED_FARTHEST (must be 1)", spec->trials);
    OI_REQUIRE(spec->reserved == 0, "narratives_seed: reserved=%u (must be 0)", spec->reserved);
    OI_CHECK(check_axis("narratives_seed", false, 0, spec->bucket_width, spec->n_buckets, "n_buckets"));
    OI_REQUIRE(seeds_out, "narratives_seed: null buffer");
    OI_CHECK(check_location("narratives_seed", location));
    std::unique_lock<std::mutex> g;
    OI_CHECK(check_index_state("narratives_seed", idx, NEED_ROWS, (filter || spec->bucket_width) ? SIMILAR_TIME_AXIS : nullptr, g));
    oi_ctx *ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    const bool host = location != OI_DEVICE;
    const size_t vb = sizeof(float) * (size_t)K * idx->dim, rb = sizeof(uint32_t) * (size_t)K;
    float *d_seeds = seeds_out;
    uint32_t *d_rows = rows_out;
    if (host) { // [seeds | rows]: the rows have their room whether or not the caller takes them
        StageLayout lay(16);
        const size_t at_seeds = lay.add(vb), at_rows = lay.add(rb);
        DevBuf &io = ctx->buf("seeds_io");
        OI_CHECK(io.ensure(lay.total()));
        d_seeds = lay.at<float>(io.p, at_seeds);
        d_rows = lay.at<uint32_t>(io.p, at_rows);
    }
    const void *d_info = nullptr;
    OI_CHECK(oi_launch_narratives_seed(idx, K, *spec, filter, d_seeds, d_rows, &d_info));
    if (host) {
        OI_HIP_CHECK(hipMemcpyAsync(seeds_out, d_seeds, vb, hipMemcpyDeviceToHost, st));
        if (rows_out) OI_HIP_CHECK(hipMemcpyAsync(rows_out, d_rows, rb, hipMemcpyDeviceToHost, st));
    }
    if (info_host) OI_HIP_CHECK(hipMemcpyAsync(info_host, d_info, sizeof(oi_seed_info), hipMemcpyDeviceToHost, st));
    if (host || info_host) OI_HIP_CHECK(hipStreamSynchronize(st));
    return OI_OK;
}

// ---- narrative terms (label_terms.hip)
static int label_terms_check_spec(const char *call, const oi_label_terms_spec *spec) {
    if (!spec) { oi_set_error("%s: null spec", call); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(spec->top >= 1 && spec->top <= OI_MAX_LABEL_TERMS, "%s: top=%u outside [1,%u]", call, spec->top, OI_MAX_LABEL_TERMS);
    OI_REQUIRE(spec->reserved[0] == 0 && spec->reserved[1] == 0, "%s: reserved=%u (must be 0)", call,
               spec->reserved[0] ? spec->reserved[0] : spec->reserved[1]);
    return OI_OK;
}
static int label_terms_check_cells(const char *call, uint32_t vocab, uint32_t K) {
    OI_REQUIRE(vocab >= 1, "%s: vocab=%u", call, vocab);
    OI_REQUIRE((uint64_t)vocab * K <= OI_MAX_LABEL_TERM_CELLS, "%s: vocab * n_clusters = %llu cells, more than %u", call,
               (unsigned long long)vocab * K, OI_MAX_LABEL_TERM_CELLS);
    return OI_OK;
}
// the handle and its state; takes the ctx lock
static int label_terms_check_index(const char *call, oi_index *idx, uint32_t K, std::unique_lock<std::mutex> &g) {
    if (!idx) { oi_set_error("%s: null index", call); return OI_ERR_INVALID_ARG; }
    OI_CHECK(label_terms_check_cells(call, idx->vocab, K));
    g = std::unique_lock<std::mutex>(idx->ctx->mu);
    return check_finalized(call, idx, false);
}

extern "C" int oi_label_term_counts(oi_index *idx, const uint32_t *labels, uint32_t K, int location, uint32_t *counts_out, uint64_t *sizes_out) {
    OI_CHECK(check_clusters("label_term_counts", K));
    OI_REQUIRE(labels && counts_out && sizes_out, "label_term_counts: null buffer");
    OI_CHECK(check_location("label_term_counts", location));
    std::unique_lock<std::mutex> g;
    OI_CHECK(label_terms_check_index("label_term_counts", idx, K, g));
    OI_HIP_CHECK(hipSetDevice(idx->ctx->device));
    if (location == OI_DEVICE) return oi_launch_label_term_counts(idx, labels, K, counts_out, sizes_out);
    return staged_call(idx->ctx, "label_terms_io", 256, {{labels, sizeof(uint32_t) * (size_t)idx->n_docs}},
                       {{counts_out, sizeof(uint32_t) * (size_t)idx->vocab * K}, {sizes_out, sizeof(uint64_t) * (size_t)K}},
                       [&](void *const *in, void *const *out) {
                           return oi_launch_label_term_counts(idx, part<const uint32_t>(in, 0), K, part<uint32_t>(out, 0), part<uint64_t>(out, 1));
                       });
}

extern "C" int oi_label_terms_rank(oi_ctx *ctx, const uint32_t *counts, const uint64_t *sizes_host, uint32_t vocab, uint32_t K,
                                   const oi_label_terms_spec *spec, int location, oi_label_term *terms_out, uint32_t *n_out) {
    static_assert(sizeof(oi_label_term) == 24 && sizeof(oi_label_terms_spec) == 16, "the records are 24 bytes, the spec 16");
    OI_CHECK(label_terms_check_spec("label_terms_rank", spec));
    OI_CHECK(check_clusters("label_terms_rank", K));
    OI_CHECK(label_terms_check_cells("label_terms_rank", vocab, K));
    OI_REQUIRE(counts && sizes_host && terms_out && n_out, "label_terms_rank: null buffer");
    unsigned long long A = 0; // (saturating: 256 sizes of 2^64 - 1 must not wrap past the check)
    for (uint32_t c = 0; c < K; ++c) A = A + sizes_host[c] < A ? ~0ull : A + sizes_host[c];
    OI_REQUIRE(A <= 0x7FFFFFFFull, "label_terms_rank: A = %llu assigned rows, more than 2^31 - 1", A);
    OI_CHECK(check_location("label_terms_rank", location));
    OI_REQUIRE(ctx, "label_terms_rank: null ctx");
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    DevBuf &ws = ctx->buf("label_terms");
    OI_CHECK(ws.ensure(oi_label_terms_rank_scratch(vocab, K, spec->top)));
    if (location == OI_DEVICE)
        return oi_launch_label_terms_rank(ctx, counts, sizes_host, nullptr, vocab, K, spec->top, spec->min_df, ws.p, terms_out, n_out);
    return staged_call(ctx, "label_terms_io", 256, {{counts, sizeof(uint32_t) * (size_t)vocab * K}},
                       {{terms_out, sizeof(oi_label_term) * (size_t)K * spec->top}, {n_out, sizeof(uint32_t) * (size_t)K}},
                       [&](void *const *in, void *const *out) {
                           return oi_launch_label_terms_rank(ctx, part<const uint32_t>(in, 0), sizes_host, nullptr, vocab, K, spec->top, spec->min_df,
                                                             ws.p, part<oi_label_term>(out, 0), part<uint32_t>(out, 1));
                       });
}

extern "C" int oi_label_terms(oi_index *idx, const uint32_t *labels, uint32_t K, const oi_label_terms_spec *spec, int location,
                              oi_label_term *terms_out, uint32_t *n_out, uint64_t *sizes_out) {
    OI_CHECK(label_terms_check_spec("label_terms", spec));
    OI_CHECK(check_clusters("label_terms", K));
    OI_REQUIRE(labels && terms_out && n_out, "label_terms: null buffer");
    OI_CHECK(check_location("label_terms", location));
    std::unique_lock<std::mutex> g;
    OI_CHECK(label_terms_check_index("label_terms", idx, K, g));
    OI_REQUIRE(idx->n_docs <= 0x7FFFFFFFull, "label_terms: n_docs=%llu, more than 2^31 - 1", (unsigned long long)idx->n_docs);
    oi_ctx *ctx = idx->ctx;
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    const uint32_t vocab = idx->vocab, top = spec->top;
    StageLayout lay(256); // [table | sizes | the rank's scratch]
    const size_t at_table = lay.add(sizeof(uint32_t) * (size_t)vocab * K), at_sizes = lay.add(sizeof(uint64_t) * (size_t)K),
                 at_scratch = lay.add(oi_label_terms_rank_scratch(vocab, K, top));
    DevBuf &ws = ctx->buf("label_terms");
    OI_CHECK(ws.ensure(lay.total()));
    // counts, rank, then the sizes to the caller (the table and the sizes never leave the device)
    auto run = [&](const uint32_t *d_labels, oi_label_term *d_terms, uint32_t *d_n, hipMemcpyKind sizes_kind) -> int {
        uint32_t *d_counts = lay.at<uint32_t>(ws.p, at_table);
        uint64_t *d_sizes = lay.at<uint64_t>(ws.p, at_sizes);
        OI_CHECK(oi_launch_label_term_counts(idx, d_labels, K, d_counts, d_sizes));
        OI_CHECK(oi_launch_label_terms_rank(ctx, d_counts, nullptr, d_sizes, vocab, K, top, spec->min_df, lay.at<void>(ws.p, at_scratch), d_terms, d_n));
        if (sizes_out) OI_HIP_CHECK(hipMemcpyAsync(sizes_out, d_sizes, sizeof(uint64_t) * (size_t)K, sizes_kind, ctx->stream));
        return OI_OK;
    };
    if (location == OI_DEVICE) return run(labels, terms_out, n_out, hipMemcpyDeviceToDevice);
    return staged_call(ctx, "label_terms_io", 256, {{labels, sizeof(uint32_t) * (size_t)idx->n_docs}},
                       {{terms_out, sizeof(oi_label_term) * (size_t)K * top}, {n_out, sizeof(uint32_t) * (size_t)K}},
                       [&](void *const *in, void *const *out) {
                           return run(part<const uint32_t>(in, 0), part<oi_label_term>(out, 0), part<uint32_t>(out, 1), hipMemcpyDeviceToHost);
                       });
}

// narrative exemplars (label_exemplars.hip)
extern "C" int oi_label_exemplars(oi_index *idx, const uint32_t *labels, const float *centroids, uint32_t K, const oi_exemplar_spec *spec,
                                  const oi_doc_filter *filter, int location, float *scores_out, uint32_t *docs_out, uint32_t *counts_out) {
    static_assert(sizeof(oi_exemplar_spec) == 16, "the spec is 16 bytes");
    if (!spec) { oi_set_error("label_exemplars: null spec"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(spec->top >= 1 && spec->top <= OI_MAX_DEPTH, "label_exemplars: top=%u outside [1,%u]", spec->top, OI_MAX_DEPTH);
    OI_REQUIRE(spec->reserved[0] == 0 && spec->reserved[1] == 0 && spec->reserved[2] == 0, "label_exemplars: reserved=%u (must be 0)",
               spec->reserved[0] ? spec->reserved[0] : spec->reserved[1] ? spec->reserved[1] : spec->reserved[2]);
    OI_CHECK(check_clusters("label_exemplars", K));
    OI_REQUIRE(labels && centroids && scores_out && docs_out && counts_out, "label_exemplars: null buffer");
    OI_CHECK(check_location("label_exemplars", location));
    std::unique_lock<std::mutex> g;
    OI_CHECK(check_index_state("label_exemplars", idx, NEED_ROWS, filter ? "a filter needs" : nullptr, g));
    OI_HIP_CHECK(hipSetDevice(idx->ctx->device));
    const uint32_t top = spec->top;
    if (location == OI_DEVICE) return oi_launch_label_exemplars(idx, labels, centroids, K, top, filter, scores_out, docs_out, counts_out);
    return staged_call(idx->ctx, "exemplars_io", 256,
                       {{labels, sizeof(uint32_t) * (size_t)idx->n_docs}, {centroids, sizeof(float) * (size_t)K * idx->dim}},
                       {{scores_out, sizeof(float) * (size_t)K * top}, {docs_out, sizeof(uint32_t) * (size_t)K * top}, {counts_out, sizeof(uint32_t) * (size_t)K}},
                       [&](void *const *in, void *const *out) {
                           return oi_launch_label_exemplars(idx, part<const uint32_t>(in, 0), part<const float>(in, 1), K, top, filter,
                                                            part<float>(out, 0), part<uint32_t>(out, 1), part<uint32_t>(out, 2));
                       });
}

// narrative breakdown (label_summary.hip)
extern "C" int oi_label_summary(oi_index *idx, const uint32_t *labels, uint32_t K, const oi_label_summary_spec *spec, const oi_doc_filter *filter,
                                int location, oi_social_counters *records_out, uint32_t *keys_out, uint32_t *counts_out,
                                uint32_t *qualified_out) {
    static_assert(sizeof(oi_label_summary_spec) == 32, "the spec is 32 bytes");
    if (!spec) { oi_set_error("label_summary: null spec"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(spec->axis == OI_LABEL_AXIS_TIME || spec->axis == OI_LABEL_AXIS_KEY, "label_summary: axis=%u is not an OI_LABEL_AXIS_* value",
               spec->axis);
    const bool key_axis = spec->axis == OI_LABEL_AXIS_KEY;
    OI_REQUIRE(spec->reserved == 0, "label_summary: reserved=%u (must be 0)", spec->reserved);
    OI_CHECK(check_axis("label_summary", key_axis, spec->stamp_origin, spec->bucket_width, spec->n_cells, "n_cells"));
    if (key_axis) OI_REQUIRE(spec->top <= OI_MAX_DEPTH, "label_summary: top=%u outside [0,%u]", spec->top, OI_MAX_DEPTH);
    else OI_REQUIRE(spec->top == 0, "label_summary: top=%u on the time axis (ranked output is the key axis's)", spec->top);
    OI_REQUIRE(spec->rank_by <= OI_GROUP_RANK_BEARISH, "label_summary: rank_by=%u is not an OI_GROUP_RANK_* value", spec->rank_by);
    OI_REQUIRE(spec->top != 0 || spec->rank_by == 0, "label_summary: rank_by=%u with top=0 (must be 0)", spec->rank_by);
    OI_CHECK(check_clusters("label_summary", K));
    OI_REQUIRE((uint64_t)K * spec->n_cells <= OI_MAX_GROUP_CELLS, "label_summary: n_clusters * n_cells = %llu cells, more than %u",
               (unsigned long long)K * spec->n_cells, OI_MAX_GROUP_CELLS);
    OI_REQUIRE(labels && records_out, "label_summary: null buffer");
    OI_REQUIRE(spec->top == 0 || (keys_out && counts_out), "label_summary: null buffer (keys_out / counts_out with top=%u)", spec->top);
    OI_CHECK(check_location("label_summary", location));
    std::unique_lock<std::mutex> g;
    OI_CHECK(check_index_state("label_summary", idx, NEED_SIGNALS,
                               key_axis ? "the key axis needs" : (filter || spec->bucket_width) ? SIMILAR_TIME_AXIS : nullptr, g));
    OI_HIP_CHECK(hipSetDevice(idx->ctx->device));
    const uint32_t top = spec->top;
    if (location == OI_DEVICE)
        return oi_launch_label_summary(idx, labels, K, *spec, filter, records_out, top ? keys_out : nullptr, top ? counts_out : nullptr,
                                       top ? qualified_out : nullptr);
    const size_t per_c = top ? top : spec->n_cells; // records (and, ranked, keys) per cluster
    const size_t kb = top ? sizeof(uint32_t) * (size_t)K * per_c : 0, cb = top ? sizeof(uint32_t) * (size_t)K : 0;
    return staged_call(idx->ctx, "label_summary_io", 256, {{labels, sizeof(uint32_t) * (size_t)idx->n_docs}},
                       {{records_out, sizeof(oi_social_counters) * (size_t)K * per_c}, {keys_out, kb}, {counts_out, cb}, {qualified_out, cb}},
                       [&](void *const *in, void *const *out) { // (dense: keys, counts and qualified are absent)
                           return oi_launch_label_summary(idx, part<const uint32_t>(in, 0), K, *spec, filter, part<oi_social_counters>(out, 0),
                                                          part<uint32_t>(out, 1), part<uint32_t>(out, 2), top && qualified_out ? part<uint32_t>(out, 3) : nullptr);
                       });
}

// ---------------------------------------------------------------- diagnostics of the bf16 screen
extern "C" int oi_screen_probe(oi_index *idx, const float *query_vecs, uint32_t B, uint64_t row_begin, uint32_t n_rows,
                               float *screen_scores_out, float *eps_out) {
    if (!idx || !query_vecs) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(B >= 1 && B <= 4096, "screen probe: n_queries=%u outside [1,4096]", B);
    OI_REQUIRE(idx->rows, "screen probe: the index holds no f32 rows");
    OI_REQUIRE(idx->dim % 16 == 0, "screen probe: dim %u is not a multiple of 16", idx->dim);
    OI_REQUIRE(row_begin <= idx->n_docs && n_rows <= idx->n_docs - row_begin && n_rows <= (1u << 20),
               "screen probe: rows [%llu, +%u) outside the index (or more than 2^20)", (unsigned long long)row_begin, n_rows);
    oi_ctx *ctx = idx->ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t n_padded = (B + 31u) & ~31u;
    DevBuf &qf = ctx->buf("probe_q"), &qb = ctx->buf("probe_q_bf16"), &ws = ctx->buf("probe_state"), &out = ctx->buf("probe_out");
    OI_CHECK(qf.ensure(sizeof(float) * (size_t)B * idx->dim));
    OI_CHECK(qb.ensure(sizeof(uint16_t) * (size_t)(n_padded + 64) * idx->dim));
    OI_CHECK(ws.ensure(sizeof(float) * (size_t)B + 16));
    OI_CHECK(out.ensure(sizeof(float) * ((size_t)B * n_rows + 1)));
    OI_HIP_CHECK(hipMemcpyAsync(qf.p, query_vecs, sizeof(float) * (size_t)B * idx->dim, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemsetAsync(ws.p, 0, sizeof(float) * (size_t)B + 16, st));
    float *eps2 = ws.as<float>();
    uint32_t *gate = reinterpret_cast<uint32_t *>(eps2 + B);
    OI_CHECK(oi_launch_screen_stage(ctx, qf.as<float>(), B, idx->dim, idx->max_row_norm.as<uint32_t>(), qb.as<uint16_t>(), eps2, gate));
    if (screen_scores_out && n_rows) {
        OI_CHECK(oi_launch_screen_probe(ctx, idx->rows, row_begin, n_rows, idx->dim, qb.as<uint16_t>(), B, out.as<float>()));
        OI_HIP_CHECK(hipMemcpyAsync(screen_scores_out, out.p, sizeof(float) * (size_t)B * n_rows, hipMemcpyDeviceToHost, st));
    }
    if (eps_out) OI_HIP_CHECK(hipMemcpyAsync(eps_out, eps2, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipStreamSynchronize(st));
    if (eps_out)
        for (uint32_t i = 0; i < B; ++i) eps_out[i] *= 0.5f; // the kernel stores the margin 2 eps
    return OI_OK;
}

// ---------------------------------------------------------------- packed multi-GPU exchange
static int search_lists_packed_impl(oi_index *idx, const float *qv, const uint32_t *qt, const uint32_t *qo,
                                    uint32_t B, uint32_t depth, int location, uint32_t *packed_out, const oi_doc_filter *filters) {
    OI_CHECK(check_search_args(idx, qv, qo, B, depth));
    OI_REQUIRE(packed_out, "search_lists_packed: null output buffer");
    SearchCall c;
    OI_CHECK(open_search(c, idx, qv, qt, qo, B, location, filters));
    oi_ctx *ctx = c.ctx;
    const size_t bytes = SearchLists::packed_bytes(B, depth);
    uint32_t *d_out = packed_out;
    if (location != OI_DEVICE) {
        DevBuf &o = ctx->buf("packed_out");
        OI_CHECK(o.ensure(bytes));
        d_out = o.as<uint32_t>();
    }
    const SearchLists l = SearchLists::packed(d_out, B, depth);
    auto body = [&]() -> int {
        OI_CHECK(l.clear_counts(B, ctx->stream));
        return l.run(idx, c, B, depth);
    };
    if (location == OI_DEVICE) return run_captured(ctx, search_graph_key(idx, c, 1, B, depth, packed_out, 0, idx->max_query_terms, 0).w, body);
    OI_CHECK(body());
    OI_HIP_CHECK(hipMemcpyAsync(packed_out, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return check_overflow_locked(ctx);
}
extern "C" int oi_search_lists_packed(oi_index *idx, const float *qv, const uint32_t *qt, const uint32_t *qo,
                                      uint32_t B, uint32_t depth, int location, uint32_t *packed_out) {
    return search_lists_packed_impl(idx, qv, qt, qo, B, depth, location, packed_out, nullptr);
}
extern "C" int oi_search_lists_packed_filtered(oi_index *idx, const float *qv, const uint32_t *qt, const uint32_t *qo,
                                               uint32_t B, uint32_t depth, const oi_doc_filter *filters, int location,
                                               uint32_t *packed_out) {
    return search_lists_packed_impl(idx, qv, qt, qo, B, depth, location, packed_out, filters);
}

// All shards' packed lists (device) -> global top-depth per list -> RRF top-k into device outputs.  ctx->mu held.
static int fuse_packed_device(oi_ctx *ctx, const uint32_t *d_in, uint32_t n_shards, uint32_t B, uint32_t depth, uint32_t k,
                              float *o_s, uint32_t *o_d, uint32_t *o_c) {
    hipStream_t st = ctx->stream;
    const size_t W = (size_t)OI_PACKED_WORDS(B, depth);
    DevBuf &flag = ctx->buf("state_flag");
    if (!flag.p) {
        OI_CHECK(flag.ensure(16));
        OI_HIP_CHECK(hipMemsetAsync(flag.p, 0, 16, st));
    }
    const uint32_t carry_cap = OI_MAX_DEPTH;
    const uint64_t mstride = (uint64_t)carry_cap + (uint64_t)n_shards * depth;
    DevBuf &pk = ctx->buf("merge_pool"), &pc = ctx->buf("merge_counts"), &ml = ctx->buf("merged_lists");
    OI_CHECK(pk.ensure(sizeof(uint64_t) * (size_t)2 * B * mstride));
    OI_CHECK(pc.ensure(sizeof(uint32_t) * (size_t)2 * B * (1 + n_shards)));
    OI_CHECK(ml.ensure(SearchLists::packed_bytes(B, depth)));
    PoolView pool{pk.as<uint64_t>(), pc.as<uint32_t>(), pc.as<uint32_t>() + 2 * (size_t)B, nullptr, mstride,
                  carry_cap, depth, n_shards, n_shards, flag.as<uint32_t>()};
    // the first shard's lists (read only) and the merged lists, both in the packed layout: scores[2][B][depth] is [2B][depth], so
    // both lists of every query are merged by ONE pair of launches (2B virtual queries; list 0 = cosine, 1 = BM25)
    const SearchLists in = SearchLists::packed(const_cast<uint32_t *>(d_in), B, depth), m = SearchLists::packed(ml.as<uint32_t>(), B, depth);
    OI_CHECK(oi_launch_lists_to_pool(ctx, in.cos_s, in.cos_d, in.cos_c, W, W, n_shards, 2 * B, depth, pool));
    OI_CHECK(oi_launch_select(ctx, pool, 2 * B, depth, false, m.cos_s, m.cos_d, m.cos_c, depth));
    return oi_launch_rrf(ctx, m.cos_d, m.cos_c, m.bm_d, m.bm_c, B, depth, k, o_s, o_d, o_c);
}
// ... into the zeroed result block of the "fuse_out" workspace: what the host tails of oi_fuse_packed and oi_search_sharded share.
// They part at the copy out (three DMAs and no overflow check / one DMA and the check); oi_pipeline_submit's tail: pipeline.hip.
static int fuse_packed_to_block(oi_ctx *ctx, const uint32_t *d_in, uint32_t n_shards, uint32_t B, uint32_t depth, uint32_t k,
                                ResultBlock *out) {
    DevBuf &fo = ctx->buf("fuse_out");
    OI_CHECK(fo.ensure(ResultBlock::bytes(B, k) + 64));
    *out = ResultBlock(fo.p, B, k);
    OI_HIP_CHECK(hipMemsetAsync(fo.p, 0, out->bytes(), ctx->stream));
    return fuse_packed_device(ctx, d_in, n_shards, B, depth, k, out->scores, out->docs, out->counts);
}

extern "C" int oi_fuse_packed(oi_ctx *ctx, const uint32_t *packed_all, uint32_t n_shards, uint32_t B, uint32_t depth,
                              uint32_t k, int location, float *scores_out, uint32_t *docs_out, uint32_t *counts_out) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(packed_all && scores_out && docs_out && counts_out, "fuse_packed: null buffer");
    OI_REQUIRE(n_shards >= 1 && n_shards <= 1024, "fuse_packed: n_shards=%u outside [1,1024]", n_shards);
    OI_REQUIRE(depth >= 1 && depth <= OI_MAX_DEPTH && k >= 1 && k <= OI_MAX_DEPTH, "fuse_packed: depth/k out of range");
    if (B == 0) return OI_OK;
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    if (location == OI_DEVICE) {
        const uint64_t key[10] = {0xF05Eull << 32, 2, (uint64_t)(uintptr_t)packed_all, ((uint64_t)n_shards << 32) | B,
                                  ((uint64_t)depth << 32) | k, (uint64_t)(uintptr_t)scores_out, (uint64_t)(uintptr_t)docs_out,
                                  (uint64_t)(uintptr_t)counts_out, 0, 0};
        return run_captured(ctx, key, [&]() -> int {
            return fuse_packed_device(ctx, packed_all, n_shards, B, depth, k, scores_out, docs_out, counts_out);
        });
    }
    const size_t in_bytes = SearchLists::packed_bytes(B, depth) * n_shards;
    DevBuf &in = ctx->buf("packed_in");
    OI_CHECK(in.ensure(in_bytes));
    OI_HIP_CHECK(hipMemcpyAsync(in.p, packed_all, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    ResultBlock r(nullptr, B, k);
    OI_CHECK(fuse_packed_to_block(ctx, in.as<uint32_t>(), n_shards, B, depth, k, &r));
    return results_to_host_direct(ctx, r, scores_out, docs_out, counts_out);
}

// ---------------------------------------------------------------- the sharded query with RCCL inside (comm.hip)
extern "C" int oi_comm_unique_id(uint8_t *id_out) {
    if (!id_out) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    return oi_rccl_unique_id(id_out);
}

extern "C" int oi_comm_create(oi_ctx *ctx, const uint8_t *id, uint32_t rank, uint32_t world, oi_comm **out) {
    if (!ctx || !id || !out) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    *out = nullptr;
    OI_REQUIRE(world >= 1 && world <= 1024 && rank < world, "comm: rank %u of %u", rank, world);
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device)); // RCCL binds the communicator to the current device
    void *nc = nullptr;
    OI_CHECK(oi_rccl_init(&nc, world, id, rank));
    oi_comm *c = new oi_comm();
    c->ctx = ctx;
    ctx->refs.fetch_add(1);
    c->nccl = nc;
    c->rank = rank;
    c->world = world;
    *out = c;
    return OI_OK;
}

extern "C" void oi_comm_destroy(oi_comm *comm) {
    if (!comm) return;
    oi_ctx *ctx = comm->ctx;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        oi_rccl_destroy(comm->nccl);
    }
    delete comm;
    ctx_release(ctx);
}

extern "C" int oi_index_finalize_sharded(oi_index *idx, oi_comm *comm) {
    if (!idx || !comm) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    if (idx->is_view) { oi_set_error("index view: read-only (set the data on the index it was taken from)"); return OI_ERR_STATE; }
    oi_ctx *ctx = idx->ctx;
    OI_REQUIRE(comm->ctx == ctx, "finalize_sharded: the communicator belongs to another context");
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!idx->forward_set) { oi_set_error("index: set_forward has not been called"); return OI_ERR_STATE; }
    if (idx->finalized) { oi_set_error("index: already finalized"); return OI_ERR_STATE; }
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // BM25 needs the statistics of the WHOLE collection: sum over the shards of (n_docs, tokens) and of df
    DevBuf &ws = ctx->buf("sharded_stats");
    OI_CHECK(ws.ensure(16 + sizeof(uint32_t) * (size_t)idx->vocab));
    uint64_t mine[2] = {idx->n_docs, idx->total_tokens};
    OI_HIP_CHECK(hipMemcpyAsync(ws.p, mine, 16, hipMemcpyHostToDevice, st));
    uint32_t *d_df = reinterpret_cast<uint32_t *>(ws.as<uint8_t>() + 16);
    OI_HIP_CHECK(hipMemcpyAsync(d_df, idx->df_local.p, sizeof(uint32_t) * (size_t)idx->vocab, hipMemcpyDeviceToDevice, st));
    OI_CHECK(oi_rccl_all_reduce_sum(comm->nccl, ws.p, 2, /*u64=*/true, st));
    OI_CHECK(oi_rccl_all_reduce_sum(comm->nccl, d_df, idx->vocab, /*u64=*/false, st));
    uint64_t glob[2] = {0, 0};
    std::vector<uint32_t> gdf(idx->vocab);
    OI_HIP_CHECK(hipMemcpyAsync(glob, ws.p, 16, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipMemcpyAsync(gdf.data(), d_df, sizeof(uint32_t) * (size_t)idx->vocab, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipStreamSynchronize(st));
    OI_CHECK(oi_bm25_finalize(idx, glob[0], glob[1], gdf.data()));
    return apply_screen_copy_policy(idx);
}

static int search_sharded_impl(oi_index *idx, oi_comm *comm, const float *qv, const uint32_t *qt, const uint32_t *qo,
                               uint32_t B, uint32_t depth, uint32_t k, int location, float *scores_out,
                               uint32_t *docs_out, uint32_t *counts_out, const oi_doc_filter *filters) {
    OI_CHECK(check_search_args(idx, qv, qo, B, depth));
    if (!comm) { oi_set_error("null communicator"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(k >= 1 && k <= OI_MAX_DEPTH, "search: k=%u outside [1,%u]", k, OI_MAX_DEPTH);
    OI_REQUIRE(scores_out && docs_out && counts_out, "search: null output buffer");
    OI_REQUIRE(comm->ctx == idx->ctx, "search_sharded: the communicator belongs to another context");
    SearchCall c;
    OI_CHECK(open_search(c, idx, qv, qt, qo, B, location, filters));
    oi_ctx *ctx = c.ctx;
    const size_t bytes = SearchLists::packed_bytes(B, depth);
    DevBuf &pk = ctx->buf("sharded_packed"), &fl = ctx->buf("sharded_flat");
    OI_CHECK(pk.ensure(bytes));
    OI_CHECK(fl.ensure(bytes * comm->world));
    const SearchLists l = SearchLists::packed(pk.as<uint32_t>(), B, depth);
    OI_CHECK(l.clear_counts(B, ctx->stream));
    OI_CHECK(l.run(idx, c, B, depth));
    // the ONE exchange per batch: every rank's packed lists to every rank (1 MB per rank at B=64, k'=1000)
    OI_CHECK(oi_rccl_all_gather_u32(comm->nccl, pk.as<uint32_t>(), fl.as<uint32_t>(), bytes / 4, ctx->stream));
    if (location == OI_DEVICE)
        return fuse_packed_device(ctx, fl.as<uint32_t>(), comm->world, B, depth, k, scores_out, docs_out, counts_out);
    ResultBlock r(nullptr, B, k);
    OI_CHECK(fuse_packed_to_block(ctx, fl.as<uint32_t>(), comm->world, B, depth, k, &r));
    OI_CHECK(results_to_host(ctx, r, scores_out, docs_out, counts_out));
    return check_overflow_locked(ctx);
}
extern "C" int oi_search_sharded(oi_index *idx, oi_comm *comm, const float *qv, const uint32_t *qt, const uint32_t *qo,
                                 uint32_t B, uint32_t depth, uint32_t k, int location, float *scores_out,
                                 uint32_t *docs_out, uint32_t *counts_out) {
    return search_sharded_impl(idx, comm, qv, qt, qo, B, depth, k, location, scores_out, docs_out, counts_out, nullptr);
}
extern "C" int oi_search_sharded_filtered(oi_index *idx, oi_comm *comm, const float *qv, const uint32_t *qt, const uint32_t *qo,
                                          uint32_t B, uint32_t depth, uint32_t k, const oi_doc_filter *filters, int location,
                                          float *scores_out, uint32_t *docs_out, uint32_t *counts_out) {
    return search_sharded_impl(idx, comm, qv, qt, qo, B, depth, k, location, scores_out, docs_out, counts_out, filters);
}
