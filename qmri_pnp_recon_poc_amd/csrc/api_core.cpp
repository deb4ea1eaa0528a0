// api_core.cpp -- the knobs, error reporting, the context's life cycle (create, destroy, stream, synchronise), the memory statistics and the
// profile chain of libqmri.so.  The gridded operator lives in api_operator.cpp, its x-update in api_xupdate.cpp.
#include "qmri_internal.h"

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <mutex>

static thread_local std::string g_create_err;

// ---------------------------------------------------------------------------------------------------
// knobs (qmri_internal.h QmriKnob): A/B and diagnostic switches behind ONE environment variable and one entry point
// ---------------------------------------------------------------------------------------------------
namespace {
struct KnobDef { QmriKnob id; const char* name; int dflt; };
constexpr KnobDef g_knob_defs[] = {
    {K_CONV_SCHEME, "conv_scheme", 2}, {K_CONV_F32, "conv_f32", 0}, {K_CONV_WT, "conv_wt", 1}, {K_CONV_XCD, "conv_xcd", 1}, {K_CONV_PERSIST, "conv_persist", 1},
    {K_CONV_SPLITK, "conv_splitk", 1}, {K_CONV_MIDCFG, "conv_midcfg", 3}, {K_CONV_DEEPCFG, "conv_deepcfg", 3}, {K_CONV_DEEPKS, "conv_deepks", 4},
    {K_CONV_RESIDENT, "conv_resident", 1}, {K_RES_HEAD, "res_head", 1}, {K_RES_TAIL, "res_tail", 1}, {K_RES_DOWN, "res_down", 1}, {K_RES_DELAY, "res_delay", 24},
    {K_RES_PIPE, "res_pipe", 1}, {K_RES_PIPE_DELAY, "res_pipe_delay", 8}, {K_RES_REARM, "res_rearm", 64},
    {K_RES_STAMPS, "res_stamps", 0}, {K_CONV_STAMPS, "conv_stamps", 0}, {K_CONV_STAMP_LAUNCH, "conv_stamp_launch", -1}, {K_LSQR_STAMPS, "lsqr_stamps", 0},
    {K_CONV_MT2, "conv_mt2", 1024}, {K_CONV_OCC, "conv_occ", 2},
    {K_FUSE_EW, "fuse_ew", 1}, {K_LSQR_PERSIST, "lsqr_persist", 1}, {K_LSQR_FOLD, "lsqr_fold", 1}, {K_DICTW_LSP, "dictw_lsp", 2}, {K_VERBOSE, "verbose", 0},
    {K_PACK_GPU, "pack_gpu", 1}, {K_NUFFT_SEG, "nufft_seg", NU_SEG},
    {K_FMAP_FUSE, "fmap_fuse", 0}, {K_FMAP_START, "fmap_start", 0}, {K_B1_SCRATCH_MB, "b1_scratch_mb", 256},
};
constexpr bool knob_defs_follow_enum() {
    if (sizeof(g_knob_defs) / sizeof(g_knob_defs[0]) != K_COUNT) return false;
    for (int k = 0; k < K_COUNT; ++k) if (g_knob_defs[k].id != k) return false;
    return true;
}
static_assert(knob_defs_follow_enum(), "g_knob_defs: one entry per QmriKnob, in the enum's order");
std::atomic<int> g_knob_val[K_COUNT];
std::once_flag g_knob_once;

int knob_index(const char* name, size_t len) {
    for (int k = 0; k < K_COUNT; ++k)
        if (strlen(g_knob_defs[k].name) == len && strncmp(g_knob_defs[k].name, name, len) == 0) return k;
    return -1;
}
void knob_init() {
    for (int k = 0; k < K_COUNT; ++k) g_knob_val[k].store(g_knob_defs[k].dflt, std::memory_order_relaxed);
    const char* e = getenv("QMRI_DEBUG");                          // the library's only environment variable
    while (e && *e) {
        const char* end = strchr(e, ',');
        const size_t len = end ? (size_t)(end - e) : strlen(e);
        const char* eq = (const char*)memchr(e, '=', len);
        const int k = eq ? knob_index(e, (size_t)(eq - e)) : -1;
        if (k >= 0) g_knob_val[k].store(atoi(eq + 1), std::memory_order_relaxed);
        else if (len) fprintf(stderr, "libqmri: QMRI_DEBUG: unknown or malformed entry '%.*s' ignored\n", (int)len, e);
        e = end ? end + 1 : nullptr;
    }
}
}  // namespace

int qmri_knob(QmriKnob k) {
    std::call_once(g_knob_once, knob_init);
    return g_knob_val[k].load(std::memory_order_relaxed);
}

extern "C" int qmri_debug_knob(const char* name, int value) {
    std::call_once(g_knob_once, knob_init);
    const int k = name ? knob_index(name, strlen(name)) : -1;
    if (k < 0) { qmri_set_error(nullptr, "qmri_debug_knob: unknown knob '%s'", name ? name : "(null)"); return QMRI_ERR_INVALID_ARG; }
    g_knob_val[k].store(value, std::memory_order_relaxed);
    return QMRI_OK;
}

void qmri_set_error(qmri_ctx* ctx, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_err = buf;
}

extern "C" int qmri_abi_version(void) { return QMRI_ABI_VERSION; }

extern "C" const char* qmri_last_error(const qmri_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

extern "C" int qmri_create(int device, qmri_ctx** out) {
    if (!out) { qmri_set_error(nullptr, "qmri_create: out is NULL"); return QMRI_ERR_INVALID_ARG; }
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        qmri_set_error(nullptr, "no HIP device available (%s); libqmri has no CPU fallback",
                       e != hipSuccess ? hipGetErrorString(e) : "device count 0");
        return QMRI_ERR_HIP;
    }
    if (device < 0 || device >= ndev) {
        qmri_set_error(nullptr, "device %d out of range (0..%d)", device, ndev - 1);
        return QMRI_ERR_INVALID_ARG;
    }
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) {
        qmri_set_error(nullptr, "hipGetDeviceProperties failed: %s", hipGetErrorString(e));
        return QMRI_ERR_HIP;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        qmri_set_error(nullptr, "device %d is %s; libqmri is built for gfx950 (MI355X) only", device, prop.gcnArchName);
        return QMRI_ERR_UNSUPPORTED;
    }
    if ((e = hipSetDevice(device)) != hipSuccess) {
        qmri_set_error(nullptr, "hipSetDevice failed: %s", hipGetErrorString(e));
        return QMRI_ERR_HIP;
    }
    qmri_ctx* ctx = new (std::nothrow) qmri_ctx();
    if (!ctx) { qmri_set_error(nullptr, "out of host memory"); return QMRI_ERR_NOMEM; }
    ctx->device = device;
    ctx->ncu = prop.multiProcessorCount;
    if ((e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking)) != hipSuccess) {
        qmri_set_error(nullptr, "hipStreamCreate failed: %s", hipGetErrorString(e));
        delete ctx;
        return QMRI_ERR_HIP;
    }
    ctx->stream = ctx->own_stream;
    for (auto& ev : ctx->ev) {
        if ((e = hipEventCreate(&ev)) != hipSuccess) {
            qmri_set_error(nullptr, "hipEventCreate failed: %s", hipGetErrorString(e));
            for (auto& x : ctx->ev) if (x) (void)hipEventDestroy(x);
            (void)hipStreamDestroy(ctx->own_stream);
            delete ctx;
            return QMRI_ERR_HIP;
        }
    }
    *out = ctx;
    return QMRI_OK;
}

int qmri_stream_idle(qmri_ctx* ctx) {
    if (ctx) QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

static MemCount g_mem_count[2];
MemCount& qmri_mem_count(bool pinned) { return g_mem_count[pinned ? 1 : 0]; }

extern "C" int qmri_debug_mem_stats(qmri_mem_stats* out) {
    if (!out) return QMRI_ERR_INVALID_ARG;
    const MemCount &d = g_mem_count[0], &h = g_mem_count[1];
    *out = qmri_mem_stats{d.live.load(), d.bytes.load(), d.total.load(), h.live.load(), h.bytes.load(), h.total.load()};
    return QMRI_OK;
}

extern "C" int qmri_destroy(qmri_ctx* ctx) {
    if (!ctx) return QMRI_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    qmri_free_operator(ctx);
    qmri_free_net(ctx);
    qmri_free_dict(ctx);
    ctx->cc = CcWork();
    for (auto& ev : ctx->ev) if (ev) (void)hipEventDestroy(ev);
    if (ctx->ev_state) (void)hipEventDestroy(ctx->ev_state);
    for (hipEvent_t e : ctx->chain) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->marks) if (e) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return QMRI_OK;
}

extern "C" int qmri_set_stream(qmri_ctx* ctx, void* hip_stream) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return QMRI_OK;
}

extern "C" int qmri_synchronize(qmri_ctx* ctx) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return QMRI_OK;
}

// profile level 2: the next (start, stop) event pair of the current chain.  The events take the timestamps of a kernel's own dispatch packet
// (hipExtLaunchKernelGGL) -- the duration rocprofv3 --kernel-trace reports -- or, with start on one launch and stop on a later one, the span
// from the first kernel's start to the last one's end (a split-K layer: convolution + reduce).  `kind` says which accumulator of qmri_profile
// the duration goes to, `flop` is the pair's fp32-equivalent algorithmic work (convolutions).
int qmri_prof_pair(qmri_ctx* ctx, hipEvent_t* start, hipEvent_t* stop, int kind, double flop) {
    *start = *stop = nullptr;
    if (ctx->prof_level < 2) return QMRI_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return QMRI_OK;
    while (ctx->chain.size() < ctx->chain_n + 2) {
        hipEvent_t e = nullptr;
        QMRI_HIP(ctx, hipEventCreate(&e));
        ctx->chain.push_back(e);
    }
    *start = ctx->chain[ctx->chain_n];
    *stop = ctx->chain[ctx->chain_n + 1];
    const size_t i = ctx->chain_n / 2;
    if (ctx->chain_kind.size() < i + 1) { ctx->chain_kind.resize(i + 1, PROF_CONV3); ctx->chain_flop.resize(i + 1, 0.0); }
    ctx->chain_kind[i] = kind;
    ctx->chain_flop[i] = flop;
    ctx->chain_n += 2;
    return QMRI_OK;
}

// synchronises and adds the chain's durations to the profile; count >= 0: only the first `count` pairs (the others are dropped)
int qmri_prof_chain_finish(qmri_ctx* ctx, long count) {
    if (ctx->prof_level < 2 || ctx->chain_n == 0) return QMRI_OK;
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i + 1 < ctx->chain_n; i += 2) {
        if (count >= 0 && (long)(i / 2) >= count) break;
        float ms = 0.f;
        QMRI_HIP(ctx, hipEventElapsedTime(&ms, ctx->chain[i], ctx->chain[i + 1]));
        const double flop = ctx->chain_flop[i / 2];
        switch (ctx->chain_kind[i / 2]) {
            case PROF_TV: ctx->prof.ms_tv_iter += ms; ctx->prof.n_tv_iter += 1; break;
            case PROF_LSQR: ctx->prof.ms_lsqr_kernels += ms; ctx->prof.n_lsqr_launches += 1; break;
            case PROF_CONV2: ctx->prof.ms_conv2x2 += ms; ctx->prof.n_conv2x2 += 1; ctx->prof.flop_conv2x2 += flop; break;
            default: ctx->prof.ms_conv3x3 += ms; ctx->prof.n_conv3x3 += 1; ctx->prof.flop_conv3x3 += flop; break;
        }
    }
    ctx->chain_n = 0;
    return QMRI_OK;
}

extern "C" int qmri_profile_enable(qmri_ctx* ctx, int level) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    ctx->prof_level = level;
    return QMRI_OK;
}

extern "C" int qmri_profile_get(qmri_ctx* ctx, qmri_profile* out, int reset) {
    if (!ctx || !out) return QMRI_ERR_INVALID_ARG;
    *out = ctx->prof;
    if (reset) ctx->prof = qmri_profile();
    return QMRI_OK;
}
