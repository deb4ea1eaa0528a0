// api_net.cpp -- denoiser plugin (param.net) of libqmri.so: weight packing, the scheme probe, the range guards, the forward pass.
// (Every QMRI_TIMING_ONLY switch of the host code is in this file: tools/build_timing_only.sh recompiles it alone.)
//
// Replaces (reference file:line): param.net main_recon_tsmis_FFT.m:138-171 + denoiseImage_PnP_ADMM.m:1-117.
// UNetRes layer order follows state_dict() of network_unet.py:68-117.
#include "qmri_internal.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

extern "C" size_t qmri_net_nparams(const qmri_net_desc* d) {
    return d ? net_plan_nparams(*d) : 0;
}

void qmri_free_net(qmri_ctx* ctx) {
    ctx->net = NetPlan();
}

// zero-initialised padded activation tensor of the layer program; Cal channels are allocated (>= C, net_plan.h; the extra ones stay zero forever
// because kernels only ever write channels < C and plane interiors), plus slack for tiles that overhang the image
static int alloc_tensor(qmri_ctx* ctx, NetTensor id, size_t B) {
    const NetPlan& p = ctx->net;
    PTensor& t = ctx->net.ten[id];
    t.C = p.prog.chan[id]; t.Cal = p.prog.cal[id]; t.H = p.H >> nt_level(id); t.W = p.W >> nt_level(id);
    t.h0 = 32; t.hp = ((t.h0 + t.H + 1 + 31) / 32) * 32;
    const size_t count = B * t.batch_stride() + 8192;
    QMRI_TRY(ctx->net.pool.alloc(ctx, &t.p, count));
    QMRI_HIP(ctx, hipMemset(t.p, 0, count * sizeof(float)));
    return QMRI_OK;
}

static int pack_layer6(qmri_ctx* ctx, ConvLayer& L, const float* w) {
    std::vector<uint16_t> p6;
    if (L.kind == CONV_3X3 || L.kind == CONV_3X3N) conv6_plan_pack(L, w, p6);     // (conv_plan_layer renames narrow 3x3 layers)
    else conv6s_plan_pack(L, w, p6);
    QMRI_TRY(L.wp6.ensure(ctx, p6.size() * sizeof(uint16_t)));
    QMRI_HIP(ctx, hipMemcpy(L.wp6, p6.data(), p6.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return QMRI_OK;
}

static size_t layer_weight_count(const ConvLayer& L) { return (size_t)L.Cin * L.Cout * ((L.kind == CONV_3X3 || L.kind == CONV_3X3N) ? 9 : 4); }

// knob pack_gpu = 1 (default, round 6): the layer is only PLANNED here; net_pack_all_dev splits and orders every layer's weights on the device.
// pack_gpu = 0: the host packers (round 1; kept as the reference of the packing and for the sanitised host build), layer by layer.
static int add_layer(qmri_ctx* ctx, const NetStep& s, const float* blob) {
    ConvLayer L;
    conv_plan_layer(L, s.kind, s.Cin, s.Cout);
    L.w_off = s.w_off;
    L.sp6 = ctx->net.sp6;
    if (!ctx->net.d_wflat) {
        const float* w = blob + s.w_off;
        std::vector<float> packed;
        L.wp_floats = conv_pack_weights(L, w, packed);
        QMRI_TRY(L.wp.ensure(ctx, packed.size()));
        QMRI_HIP(ctx, hipMemcpy(L.wp, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
        QMRI_TRY(pack_layer6(ctx, L, w));                      // the same weights, split for the bf16 / f16 matrix-core kernels
    }
    L.index = (int)ctx->net.layers.size();
    ctx->net.layers.push_back(std::move(L));
    return QMRI_OK;
}

static int pack_layer6_dev(qmri_ctx* ctx, ConvLayer& L) {
    const NetPlan& p = ctx->net;
    const float mx = (L.index >= 0 && (size_t)L.index < p.w_max.size()) ? p.w_max[L.index] : 0.f;
    if (L.kind == CONV_3X3 || L.kind == CONV_3X3N) return conv6_pack_dev(ctx, L, p.d_wflat + L.w_off, mx);
    return conv6s_pack_dev(ctx, L, p.d_wflat + L.w_off, mx);
}

// The device side of qmri_set_denoiser's weight handling: every layer's largest |w| (the f16 scheme's per-layer scale and its range check), then
// the three packings per layer as kernels reading the flat blob in device memory.  One host synchronisation (the maxima).
static int net_pack_all_dev(qmri_ctx* ctx) {
    NetPlan& p = ctx->net;
    const size_t nl = p.layers.size();
    DevBuf<unsigned> d_max;
    QMRI_TRY(d_max.ensure(ctx, nl));
    const int rc = [&]() -> int {
        if (hipMemsetAsync(d_max, 0, nl * sizeof(unsigned), ctx->stream) != hipSuccess) return QMRI_ERR_HIP;
        for (size_t l = 0; l < nl; ++l)
            QMRI_TRY(ew_launch_absmax(ctx, p.d_wflat + p.layers[l].w_off, nullptr, layer_weight_count(p.layers[l]), d_max + l));
        std::vector<unsigned> bits(nl);
        if (hipMemcpyAsync(bits.data(), d_max, nl * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) return QMRI_ERR_HIP;
        p.w_max.resize(nl);
        bool fit = true;
        for (size_t l = 0; l < nl; ++l) {
            std::memcpy(&p.w_max[l], &bits[l], 4);
            if (!(p.w_max[l] <= 60000.f)) fit = false;             // (conv6_weights_fit_f16: the f16 pieces carry |w| <= 6e4; NaN too)
        }
        if (p.sp6 == 2 && !fit) p.sp6 = 3;                         // weights beyond the f16 range: bf16 scheme
        for (ConvLayer& L : p.layers) {
            L.sp6 = p.sp6;
            QMRI_TRY(conv_pack_weights_dev(ctx, L, p.d_wflat + L.w_off));
            QMRI_TRY(pack_layer6_dev(ctx, L));
        }
        return QMRI_OK;
    }();
    if (rc == QMRI_ERR_HIP && ctx->err.empty()) qmri_set_error(ctx, "HIP failure while packing the denoiser's weights on the device");
    return rc;
}

// Re-pack every layer for the other operand-splitting scheme (sp = 2: f16 x 3 products, sp = 3: bf16 x 6 products).
static int net_set_scheme(qmri_ctx* ctx, int sp) {
    NetPlan& p = ctx->net;
    if (p.sp6 == sp) return QMRI_OK;
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (ConvLayer& L : p.layers) {
        L.wp6.reset();
        L.sp6 = sp;
        if (p.d_wflat) QMRI_TRY(pack_layer6_dev(ctx, L));
        else QMRI_TRY(pack_layer6(ctx, L, p.w_host.data() + L.w_off));
    }
    if (!p.d_wflat) QMRI_HIP(ctx, hipDeviceSynchronize());         // (the host packers' copies travel on the NULL stream: see qmri_set_denoiser)
    p.sp6 = sp;
    return QMRI_OK;
}

// After a synchronisation: did a layer's output leave the range the f16 split carries (|x| <= 6e4, finite)?  If so the
// network is switched to the bf16 scheme (8 exponent bits, no range limit) and the caller runs its work again.
int net_range_tripped(qmri_ctx* ctx, bool& tripped) {
    NetPlan& p = ctx->net;
    tripped = false;
    if (p.sp6 != 2 || !p.d_range_flag) return QMRI_OK;
    unsigned f = 0;
    // (on the context's own stream: the callers have synchronised it, and the kernels of the repeated run that raise this flag again are ordered
    //  behind the reset -- a NULL-stream memset is not ordered with a non-blocking stream, see qmri_set_denoiser)
    QMRI_HIP(ctx, hipMemcpyAsync(&f, p.d_range_flag, sizeof f, hipMemcpyDeviceToHost, ctx->stream));
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
#ifdef QMRI_TIMING_ONLY
    f = 0;
#endif
    if (!f) return QMRI_OK;
    QMRI_HIP(ctx, hipMemsetAsync(p.d_range_flag, 0, sizeof f, ctx->stream));
    if (p.h_range_flag) std::memset(p.h_range_flag, 0, (size_t)p.h_range_words * sizeof(unsigned));
    tripped = true;
    if (f & 4u) {                                                   // a hand-off of the resident-tile launch timed out: its results are garbage, and so
        // may the other bits be.  Co-residency of its workgroups is assumed from tiles <= CUs; another stream, context or process on the device can break
        // it for a while (tests/test_gpu_net.py: two contexts).  The call is repeated with one launch per layer; the resident form is tried again after
        // res_rearm clean passes (knob, default 64) -- unless it has timed out three times since qmri_set_denoiser: then it stays off.
        p.res_off = true;
        p.res_timeouts += 1;
        p.res_clean = 0;
        if (p.res_timeouts <= 3)
            fprintf(stderr, "libqmri: a tile hand-off of the resident-tile convolution launch timed out (%d since set-up); repeating with one launch per layer%s\n",
                    p.res_timeouts, p.res_timeouts >= 3 ? ", the resident form stays off" : "");
        return QMRI_OK;
    }
    if (qmri_knob(K_VERBOSE)) fprintf(stderr, "libqmri: range guard of the f16 scheme tripped (flag %u: 1 overflow, 2 a layer collapsed): the network moves to the bf16 scheme\n", f);
    QMRI_TRY(net_set_scheme(ctx, 3));
    p.fallbacks += 1;
    return QMRI_OK;
}

// any bit in the pinned host words of the range guards (k_act_check, conv6_kernels.hip)
bool host_range_tripped(const NetPlan& p) {
#ifdef QMRI_TIMING_ONLY
    return false;
#endif
    if (!p.h_range_flag) return false;
    const int n = std::min(p.h_range_words, (int)p.layers.size() + 1);
    for (int i = 0; i < n; ++i) if (p.h_range_flag[i]) return true;
    return false;
}

static int net_forward_padded(qmri_ctx* ctx, int B);

// The f16 operand split represents values below ~2.4e-4 with an absolute, not a relative error.  Inputs
// are at unit scale by construction ([0, 1] in the ADMM loop, rescaled in qmri_denoise) and weights are rescaled per layer; what
// is left is the network's own gain from layer to layer.  Whether that matters for THIS network is measured once at set-up
// time: one forward on a unit-scale probe with the f16 kernels, one with the f32-MFMA kernels (their weights are packed anyway),
// and if the outputs differ by more than fp32 summation-order noise -- or the overflow guard trips -- the network runs on the
// bf16 scheme (no range limits) from the start.  (The run-time overflow guard stays: it covers inputs the probe did not see.)
static int net_calibrate_scheme(qmri_ctx* ctx) {
    NetPlan& p = ctx->net;
    struct ResOff { NetPlan& n; bool was; ~ResOff() { n.res_off = was; } } res_guard{p, p.res_off};
    p.res_off = true;                                                // (one launch per layer here: same bits, and a hand-off time-out could not be told from a range problem)
    const size_t n = (size_t)p.desc.in_nc * p.H * p.W, nout = p.ten[NT_OUT32].batch_stride();
    std::vector<float> h(n);
    uint32_t st = 0x2545F491u;
    for (size_t i = 0; i < n; ++i) { st = st * 1664525u + 1013904223u; h[i] = (float)(st >> 8) * (1.0f / 16777216.0f); }   // uniform [0, 1)
    DevBuf<float> d_tmp, d_ref;
    DevBuf<unsigned> d_m;
    const int rc = [&]() -> int {
        QMRI_TRY(d_tmp.ensure(ctx, n));
        QMRI_TRY(d_ref.ensure(ctx, nout));
        QMRI_TRY(d_m.ensure(ctx, 2));
        if (hipMemsetAsync(d_m, 0, 2 * sizeof(unsigned), ctx->stream) != hipSuccess ||
            hipMemcpyAsync(d_tmp, h.data(), n * sizeof(float), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return QMRI_ERR_HIP;
        QMRI_TRY(ew_launch_pack(ctx, 1, p.desc.in_nc, p.H, p.W, d_tmp, 0, p.ten[NT_IN32]));
        p.force_f32 = true;                                          // reference: exact fp32 products
        int st = net_forward_padded(ctx, 1);
        p.force_f32 = false;
        QMRI_TRY(st);
        if (hipMemcpyAsync(d_ref, p.ten[NT_OUT32].p, nout * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) return QMRI_ERR_HIP;
        p.act_record = true;                                         // ... which also record every layer's magnitude (ACT_LOW guard)
        st = net_forward_padded(ctx, 1);                             // the f16 kernels
        p.act_record = false;
        QMRI_TRY(st);
        QMRI_TRY(ew_launch_absmax(ctx, d_ref, nullptr, nout, d_m));
        QMRI_TRY(ew_launch_absmax(ctx, p.ten[NT_OUT32].p, d_ref, nout, d_m + 1));
        unsigned m[2] = {0, 0}, flag = 0;
        if (hipMemcpyAsync(m, d_m, sizeof m, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(&flag, p.d_range_flag, sizeof flag, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) return QMRI_ERR_HIP;
        float ref_max, diff_max;
        std::memcpy(&ref_max, &m[0], 4); std::memcpy(&diff_max, &m[1], 4);
#ifdef QMRI_TIMING_ONLY   // builds with parts of a kernel removed (tools/ab_*.sh): wrong results by design -- without this the probe would put them on the bf16 scheme
        const bool ok = true;
#else
        const bool ok = flag == 0 && std::isfinite(ref_max) && std::isfinite(diff_max) && diff_max <= 2e-5f * ref_max;
#endif
        if (qmri_knob(K_VERBOSE))
            fprintf(stderr, "libqmri: calibration probe: max |out| %.3g, max |f16 - f32| %.3g, overflow flag %u -> %s scheme\n", ref_max, diff_max, flag,
                    ok ? "f16 x 3" : "bf16 x 6");
        if (!ok) {
            if (hipMemsetAsync(p.d_range_flag, 0, sizeof flag, ctx->stream) != hipSuccess) return QMRI_ERR_HIP;
            return net_set_scheme(ctx, 3);
        }
        return QMRI_OK;
    }();
    if (rc == QMRI_ERR_HIP && ctx->err.empty()) qmri_set_error(ctx, "HIP failure in the denoiser calibration pass");
    return rc;
}

extern "C" int qmri_set_denoiser(qmri_ctx* ctx, const qmri_net_desc* desc, const float* weights, size_t nbytes, int H, int W,
                                 int max_batch) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    QMRI_CHECK_ARG(ctx, desc && weights, "desc / weights must not be NULL");
    QMRI_CHECK_ARG(ctx, H > 0 && W > 0 && max_batch > 0, "H, W, max_batch must be positive");
    QMRI_CHECK_ARG(ctx, desc->in_nc > 0 && desc->out_nc > 0 && desc->nb >= 1, "in_nc, out_nc, nb must be positive");
    if (desc->arch != QMRI_ARCH_UNETRES && desc->arch != QMRI_ARCH_SEQ_CONV) {
        qmri_set_error(ctx, "unknown network architecture %d", desc->arch);
        return QMRI_ERR_UNSUPPORTED;
    }
    if (desc->arch == QMRI_ARCH_UNETRES && (H % 8 != 0 || W % 8 != 0)) {
        // UNetRes has three 2x down-samplers and no padding logic (network_unet.py:106-117)
        qmri_set_error(ctx, "UNetRes needs H and W divisible by 8 (got %d x %d)", H, W);
        return QMRI_ERR_UNSUPPORTED;
    }
    NetProgram prog = net_plan_build(*desc);                         // the layers, their operands, the tensors' channels: everything below follows it
    if (nbytes != 4 * prog.nparams) {
        qmri_set_error(ctx, "weight blob is %zu bytes, architecture needs %zu", nbytes, 4 * prog.nparams);
        return QMRI_ERR_INVALID_ARG;
    }
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    qmri_free_net(ctx);
    NetPlan& p = ctx->net;
    p.desc = *desc; p.H = H; p.W = W; p.maxB = max_batch;
    p.prog = std::move(prog);
    p.sp6 = conv6_default_sp();
    const auto t_upload = std::chrono::steady_clock::now();
    if (qmri_knob(K_PACK_GPU)) {
        // the caller's blob goes to the device once, as it is; every packing is a kernel over it (net_pack_all_dev) and a later change of scheme re-packs from it
        QMRI_TRY(p.pool.alloc(ctx, &p.d_wflat, nbytes / 4));
        QMRI_HIP(ctx, hipMemcpyAsync(p.d_wflat, weights, nbytes, hipMemcpyHostToDevice, ctx->stream));   // (on the stream the packing kernels run on: ordered with them)
    } else {
        p.w_host.assign(weights, weights + nbytes / 4);
        if (p.sp6 == 2 && !conv6_weights_fit_f16(weights, nbytes / 4)) p.sp6 = 3;     // weights beyond the f16 range: bf16 scheme
    }
    QMRI_TRY(p.pool.alloc(ctx, &p.d_range_flag, 1));
    QMRI_HIP(ctx, hipMemset(p.d_range_flag, 0, sizeof(unsigned)));
    p.h_range_words = 4096;
    QMRI_TRY(p.h_range_flag.ensure(ctx, (size_t)p.h_range_words));
    std::memset(p.h_range_flag, 0, (size_t)p.h_range_words * sizeof(unsigned));
    const size_t B = (size_t)max_batch;
    // (qmri_get_health: where the set-up time goes -- the layers' weight packing and upload, the tensors, the calibration probe)
    typedef std::chrono::steady_clock Clk;
    const auto t_begin = Clk::now();
    double ms_pack = std::chrono::duration<double, std::milli>(t_begin - t_upload).count();      // (the blob's upload / host copy and range check)
    for (const NetStep& s : p.prog.steps) QMRI_TRY(add_layer(ctx, s, weights));
    ms_pack += std::chrono::duration<double, std::milli>(Clk::now() - t_begin).count();
    for (int id = 0; id < NT_IN32; ++id)                           // the interior tensors the architecture has, level after level
        if (p.prog.chan[id]) QMRI_TRY(alloc_tensor(ctx, (NetTensor)id, B));
    // k_conv6r's exchange buffer (one slice): where the program has runs to offer it (64 channels at full resolution: conv6r_try)
    if (!p.prog.runs.empty() && desc->nc[0] == 64 && H % 16 == 0 && W % 16 == 0 && (H / 16) * (W / 16) <= 1024) {
        p.res_tiles = (H / 16) * (W / 16);
        QMRI_TRY(p.pool.alloc(ctx, &p.d_res_xbuf, conv6r_xbuf_bytes(p.res_tiles)));
        QMRI_HIP(ctx, hipMemset(p.d_res_xbuf, 0, conv6r_xbuf_bytes(p.res_tiles)));
        p.res_epoch = 0; p.res_off = false;
        if (qmri_knob(K_RES_STAMPS)) { QMRI_TRY(p.pool.alloc(ctx, &p.d_res_stamps, 2048 * sizeof(unsigned long long))); QMRI_HIP(ctx, hipMemset(p.d_res_stamps, 0, 2048 * sizeof(unsigned long long))); }
    }
    if (p.d_wflat) {
        const auto t0 = Clk::now();
        QMRI_TRY(net_pack_all_dev(ctx));
        QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));          // (the time of the packing kernels belongs to this figure)
        ms_pack += std::chrono::duration<double, std::milli>(Clk::now() - t0).count();
    }
    QMRI_TRY(alloc_tensor(ctx, NT_IN32, B));
    QMRI_TRY(alloc_tensor(ctx, NT_OUT32, B));
    // BLOCKED interior tensors (PTensor::blk): every layer on the conv6 kernels, every interior channel count a multiple of 8 (net_plan.h)
    p.blk_ok = conv6_enabled() && p.prog.blk_ok;
    for (const ConvLayer& L : p.layers) if (!L.wp6) p.blk_ok = false;
    p.interior_fmt = -1;
    QMRI_TRY(p.pool.alloc(ctx, &p.d_counter, (size_t)1));
    QMRI_HIP(ctx, hipMemset(p.d_counter, 0, sizeof(unsigned)));
    if (qmri_knob(K_CONV_STAMPS)) { QMRI_TRY(p.pool.alloc(ctx, &p.d_stamps, 4096 * 11 * sizeof(unsigned long long))); }
    p.counter_base = 0;
    p.ready = true;
    // (device-wide: the host packers' blocking copies travel on the NULL stream, which this context's non-blocking stream is not ordered with -- beside
    //  another process on the device the set-up probe below was seen to read weights that had not landed and to choose the bf16 scheme for a network
    //  that does not need it, five times out of six: tools/probe_under_contention.py, profiles/r06_e_*)
    QMRI_HIP(ctx, hipDeviceSynchronize());
    const auto t_cal = Clk::now();
    if (p.sp6 == 2) QMRI_TRY(net_calibrate_scheme(ctx));
    const auto t_end = Clk::now();
    p.setup_ms[0] = ms_pack;
    p.setup_ms[2] = std::chrono::duration<double, std::milli>(t_end - t_cal).count();
    p.setup_ms[1] = std::chrono::duration<double, std::milli>(t_cal - t_upload).count() - ms_pack;
    return QMRI_OK;
}

// The layer program (net_plan.h), step by step: one launch per layer -- but where resident-run candidates start at a step, the first one conv6r_try
// takes runs all its member layers as ONE launch with resident tiles (the full-resolution level; knobs res_head / res_tail / res_down = 0 keep the
// head / tail / down-sampling convolution out of such a launch).
static int net_forward_layers(qmri_ctx* ctx, int B) {
    NetPlan& p = ctx->net;
    const std::vector<NetStep>& steps = p.prog.steps;
    const std::vector<NetRun>& runs = p.prog.runs;
    const bool resident = p.d_res_xbuf && !p.force_f32;
    const bool res_head = qmri_knob(K_RES_HEAD) != 0, res_tail = qmri_knob(K_RES_TAIL) != 0, res_down = qmri_knob(K_RES_DOWN) != 0;
    auto ten = [&p](NetTensor id) -> const PTensor* { return id == NT_NONE ? nullptr : &p.ten[id]; };
    auto layer = [&p](int i) -> const ConvLayer* { return i < 0 ? nullptr : &p.layers[i]; };
    size_t ri = 0;
    for (size_t i = 0; i < steps.size();) {
        bool taken = false;
        for (; !taken && ri < runs.size() && runs[ri].first <= (int)i; ++ri) {
            const NetRun& c = runs[ri];
            if (c.first != (int)i || !resident || !net_run_allowed(c, res_head, res_tail, res_down)) continue;
            Conv6rRun r;
            r.head = layer(c.head); r.head_in = ten(c.head_in); r.res = layer(c.res); r.nres = c.nres; r.src = ten(c.src); r.cur = ten(c.cur); r.skip = ten(c.skip);
            r.tail = layer(c.tail); r.tail_out = ten(c.tail_out); r.down = layer(c.down); r.down_out = ten(c.down_out);
            QMRI_TRY(conv6r_try(ctx, r, B, &taken));
            if (taken) i += (size_t)c.count;
        }
        if (taken) continue;
        const NetStep& s = steps[i];
        QMRI_TRY(conv_launch(ctx, p.layers[i], B, p.ten[s.in], p.ten[s.out], ten(s.add1), ten(s.add2), s.relu_out));
        ++i;
    }
    return QMRI_OK;
}

// network forward on the context's padded tensors: in32 -> out32
static int net_forward_padded(qmri_ctx* ctx, int B) {
    {
        // Interior tensors (everything between the head's input and the tail's output) are BLOCKED when every layer runs on the
        // matrix-core kernels (PTensor::blk), planar otherwise (the f32-MFMA kernels of the calibration pass, knob conv_f32, odd
        // channel counts).  The two formats put the zero halo at different addresses: a change of format re-zeroes the tensors.
        NetPlan& p = ctx->net;
        const bool blk = p.blk_ok && !p.force_f32 && conv6_enabled();
        const bool rezero = p.interior_fmt != -1 && p.interior_fmt != (blk ? 1 : 0);
        for (int id = 0; id < NT_IN32; ++id) {
            PTensor& t = p.ten[id];
            if (rezero && t.p) QMRI_HIP(ctx, hipMemsetAsync(t.p, 0, ((size_t)p.maxB * t.batch_stride() + 8192) * sizeof(float), ctx->stream));
            t.blk = blk;
        }
        p.interior_fmt = blk ? 1 : 0;
    }
    const bool report = !ctx->net.force_f32;                        // (the calibration's f32 pass reports nothing)
    const bool timed = ctx->prof_level >= 2;                        // profile level 2: the whole pass between two stream events (besides the per-launch pairs)
    if (timed) QMRI_HIP(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
    if (report) QMRI_TRY(conv6_act_begin(ctx, (int)ctx->net.layers.size()));
    QMRI_TRY(net_forward_layers(ctx, B));
    if (report) QMRI_TRY(conv6_act_end(ctx));                       // low-magnitude guard of the f16 scheme (conv6_kernels.hip, ACT_LOW)
    if (timed) QMRI_HIP(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
    QMRI_TRY(qmri_prof_chain_finish(ctx));                          // (level 2: synchronises)
    if (timed) {
        float ms = 0.f;
        QMRI_HIP(ctx, hipEventSynchronize(ctx->ev[3]));
        QMRI_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]));
        ctx->prof.ms_net_forward += ms; ctx->prof.n_net_forward += 1;
    }
    return QMRI_OK;
}

// (A hipGraph replay of the forward pass -- ~65 dependent launches with fixed arguments -- was measured in round 1 and is not faster: 413.7 vs 413.8
//  ADMM it/s; the 3-4 us between dependent kernels are spent on the device, not on the host.  The capture path is gone since round 5.)
int net_forward(qmri_ctx* ctx, int B) {
    NetPlan& p = ctx->net;
    const int st = net_forward_padded(ctx, B);
    // the resident-tile launch is switched off by a hand-off time-out (net_range_tripped); after K_RES_REARM clean forward passes it is tried again
    if (st == QMRI_OK && p.res_off && p.res_timeouts > 0 && p.res_timeouts < 3 && !p.res_forced_off && ++p.res_clean >= std::max(1, qmri_knob(K_RES_REARM))) {
        p.res_off = false;
        p.res_clean = 0;
    }
    return st;
}

extern "C" int qmri_net_forward_dev(qmri_ctx* ctx, const float* d_in, int B, float* d_out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    NetPlan& p = ctx->net;
    if (!p.ready) { qmri_set_error(ctx, "denoiser not set: call qmri_set_denoiser first"); return QMRI_ERR_STATE; }
    QMRI_CHECK_ARG(ctx, d_in && d_out && B >= 1 && B <= p.maxB, "qmri_net_forward_dev arguments / batch > max_batch");
    {   // the guarded second attempt reads d_in again: input and output must not overlap
        const size_t hw = (size_t)p.H * p.W * B * sizeof(float);
        const char *a = (const char*)d_in, *b = (const char*)d_out;
        QMRI_CHECK_ARG(ctx, a + hw * p.desc.in_nc <= b || b + hw * p.desc.out_nc <= a, "qmri_net_forward_dev: d_in and d_out must not overlap");
    }
    // A pass is repeated for two separate reasons -- a hand-off time-out of the resident-tile launch (then one launch per layer), the f16 range guard
    // (then the bf16 scheme) -- and one may follow the other: up to three passes, and a call that still wants another one is an error, not QMRI_OK.
    bool again = false;
    for (int attempt = 0; attempt < 3; ++attempt) {
        QMRI_TRY(ew_launch_pack(ctx, B, p.desc.in_nc, p.H, p.W, d_in, 0, p.ten[NT_IN32]));
        QMRI_TRY(net_forward(ctx, B));
        QMRI_TRY(ew_launch_unpack(ctx, B, p.desc.out_nc, p.H, p.W, p.ten[NT_OUT32], p.ten[NT_IN32], 0, d_out, 0));
        again = false;
        if (p.sp6 != 2) break;                              // (the bf16 scheme has no range to guard: stays asynchronous)
        QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        QMRI_TRY(net_range_tripped(ctx, again));
        if (!again) break;
    }
    if (again) { qmri_set_error(ctx, "the network's guards asked for a fourth pass (resident-tile hand-off / f16 range): giving up"); return QMRI_ERR_HIP; }
    return QMRI_OK;
}

// test / A-B hook: the resident-tile launch of the full-resolution ResBlocks (conv6_kernels.hip k_conv6r)
extern "C" int qmri_debug_conv_resident(qmri_ctx* ctx, int on, int* timeouts_out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    NetPlan& p = ctx->net;
    if (timeouts_out) *timeouts_out = p.res_timeouts;
    if (!p.ready) return QMRI_OK;
    p.res_off = (on == 0);
    p.res_forced_off = (on == 0);                                   // (a caller's choice is not re-armed behind its back)
    if (on) { p.res_timeouts = std::min(p.res_timeouts, 2); p.res_clean = 0; }
    p.res_drop = (on == 2) ? 1 : 0;
    return QMRI_OK;
}

extern "C" int qmri_denoiser_scheme(const qmri_ctx* ctx, int* scheme_out, int* fallbacks_out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    if (!ctx->net.ready) return QMRI_ERR_STATE;
    if (scheme_out) *scheme_out = ctx->net.sp6;
    if (fallbacks_out) *fallbacks_out = ctx->net.fallbacks;
    return QMRI_OK;
}

extern "C" int qmri_get_health(const qmri_ctx* ctx, qmri_health* out) {
    if (!ctx || !out) return QMRI_ERR_INVALID_ARG;
    const NetPlan& p = ctx->net;
    std::memset(out, 0, sizeof *out);
    out->denoiser_scheme = p.ready ? p.sp6 : 0;
    out->denoiser_fallbacks = p.ready ? p.fallbacks : 0;
    out->resident_armed = (p.ready && !p.res_off && p.sp6 == 2 && qmri_knob(K_CONV_RESIDENT) != 0) ? 1 : 0;
    out->resident_timeouts = p.res_timeouts;
    out->lsqr_one_launch = (ctx->ks_persist < 0) ? -1 : (ctx->ks_persist > 0 ? 1 : 0);
    out->lsqr_timeouts = ctx->ks_timeouts;
    out->repeated_calls = ctx->admm_repeats;
    out->last_call_wall_ms = ctx->last_call_wall_ms;
    for (int i = 0; i < 4; ++i) out->last_call_stage_ms[i] = ctx->last_call_ms[i];
    for (int i = 0; i < 3; ++i) out->set_denoiser_ms[i] = p.setup_ms[i];
    return QMRI_OK;
}

extern "C" int qmri_denoise(qmri_ctx* ctx, const double* in, int H, int W, int C, int B, double* out) {
    if (!ctx) return QMRI_ERR_INVALID_ARG;
    QMRI_HIP(ctx, hipSetDevice(ctx->device));
    NetPlan& p = ctx->net;
    if (!p.ready) { qmri_set_error(ctx, "denoiser not set: call qmri_set_denoiser first"); return QMRI_ERR_STATE; }
    QMRI_CHECK_ARG(ctx, in && out, "in / out must not be NULL");
    if (H != p.H || W != p.W || C != p.desc.in_nc) {
        // MATLAB: images:denoiseImage:incompatibleImageNetwork-style size error from activations()
        qmri_set_error(ctx, "input %d x %d x %d does not match the network input %d x %d x %d", H, W, C, p.H, p.W, p.desc.in_nc);
        return QMRI_ERR_INVALID_ARG;
    }
    QMRI_CHECK_ARG(ctx, B >= 1 && B <= p.maxB, "batch exceeds max_batch of qmri_set_denoiser");
    const size_t HW = (size_t)H * W, nin = HW * C * B, nout = HW * p.desc.out_nc * B;
    // Both architectures are bias-free convolutions + ReLU (+ skips): net(2^k x) = 2^k net(x) exactly in fp32.  Inputs far from unit
    // scale are therefore brought to [0.5, 1) by a power of two on the way in and back on the way out, so that the f16 pieces of
    // the activations stay in their normal range; inputs of ordinary scale -- the [0, 1] images of the
    // ADMM loop -- are left alone.
    float in_scale = 1.f, out_scale = 1.f;
    {
        // (four independent maxima: the loop vectorises; a NaN never raises amax -- such an input goes through unscaled and the range guard sees it)
        double m4[4] = {0.0, 0.0, 0.0, 0.0};
        size_t i = 0;
        for (; i + 4 <= nin; i += 4)
            for (int j = 0; j < 4; ++j) { const double a = std::fabs(in[i + j]); m4[j] = a > m4[j] ? a : m4[j]; }
        for (; i < nin; ++i) { const double a = std::fabs(in[i]); m4[0] = a > m4[0] ? a : m4[0]; }
        const double amax = std::max(std::max(m4[0], m4[1]), std::max(m4[2], m4[3]));
        if (std::isfinite(amax) && amax > 0.0 && (amax < 0.0625 || amax >= 256.0)) {
            int e = 0;
            (void)std::frexp(amax, &e);                             // amax = f * 2^e, f in [0.5, 1)
            const int k = std::min(100, std::max(-100, -e));
            in_scale = std::ldexp(1.f, k); out_scale = std::ldexp(1.f, -k);
        }
    }
    // staging buffer of the per-call drop-in mode (the reference's own PnP_ADMM.m calling param.net 100 times): kept with the plan, grown on demand
    QMRI_TRY(p.d_io.ensure(ctx, std::max(nin, nout)));
    double* const d_io = p.d_io;
    bool again = false;
    auto pass = [&]() -> int {
        if (hipMemcpyAsync(d_io, in, nin * sizeof(double), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return QMRI_ERR_HIP;
        QMRI_TRY(ew_launch_pack(ctx, B, C, H, W, d_io, 1, p.ten[NT_IN32], in_scale));                      // im2single: :72-77
        QMRI_TRY(net_forward(ctx, B));                                                            // activations(...): :88
        QMRI_TRY(ew_launch_unpack(ctx, B, p.desc.out_nc, H, W, p.ten[NT_OUT32], p.ten[NT_IN32], p.desc.residual_noise, d_io, 1, out_scale));
        if (hipMemcpyAsync(out, d_io, nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return QMRI_ERR_HIP;
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) return QMRI_ERR_HIP;
        return net_range_tripped(ctx, again);
    };
    int st = QMRI_OK;
    for (int attempt = 0; attempt < 3; ++attempt) {        // (further passes only after a guard changed the plan: see qmri_net_forward_dev)
        again = false;
        st = pass();
        if (st != QMRI_OK || !again) break;
    }
    if (st == QMRI_OK && again) { qmri_set_error(ctx, "the network's guards asked for a fourth pass (resident-tile hand-off / f16 range): giving up"); st = QMRI_ERR_HIP; }
    if (st == QMRI_ERR_HIP && ctx->err.empty()) qmri_set_error(ctx, "HIP failure in qmri_denoise");
    return st;
}

// diagnostic: copy the per-workgroup stamps of the most recent conv launch (see conv_kernels.hip) to the host
extern "C" int qmri_debug_conv_stamps(qmri_ctx* ctx, unsigned long long* out, int nwg) {
    if (ctx && nwg == -6 && ctx->net.d_res_stamps) {                // (the resident-tile launch's stamps: 2048 values, knob res_stamps)
        QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
        QMRI_HIP(ctx, hipMemcpy(out, ctx->net.d_res_stamps, (size_t)2048 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return QMRI_OK;
    }
    if (!ctx || !ctx->net.d_stamps) return QMRI_ERR_STATE;
    QMRI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    QMRI_HIP(ctx, hipMemcpy(out, ctx->net.d_stamps, (size_t)4096 * 11 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return QMRI_OK;
}
