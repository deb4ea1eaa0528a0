// conv6_form.h -- which kernel, pixel tile, K split and grid a 3x3 layer of the 16-bit matrix-core path gets, and why: ONE pure function,
// conv6_choose_form().  conv6_launch (conv6_kernels.hip) asks it and executes the answer; nothing else decides.  No HIP, no context: plain
// C++17, so that tests/cpp/conv6_form_test.cpp can put the function the library calls beside the tests' own restatement of it
// (tests/test_gpu_conv_layers.py launch_form) on a machine without a GPU.
#ifndef QMRI_CONV6_FORM_H          // (a guard, not #pragma once: the header is also compiled on its own)
#define QMRI_CONV6_FORM_H

// what the decision needs to know of a tensor (qmri_internal.h PTensor): present, BLOCKED format, first interior row, row pitch, plane size
struct Conv6Operand { bool on = false, blk = false; int h0 = 0, hp = 0; long plane = 0; };
struct Conv6Shape {
    int Cin, Cout, H, W, B;
    int sp6;                        // the layer's scheme: 2 = f16 x 3 products, 3 = bf16 x 6 products
    bool in_blk;                    // the input is a BLOCKED tensor
    Conv6Operand out, add1, add2;   // the output and the optional residual operands
};
struct Conv6Knobs { int conv_splitk = 1, conv_persist = 1, conv_midcfg = 3, conv_deepcfg = 3, conv_deepks = 4; };   // (defaults: api_core.cpp)

enum Conv6Kernel { CONV6_KERNEL_CONV6 = 0, CONV6_KERNEL_CONV6P = 1 };   // one workgroup per tile | one workgroup per CU walks the tiles
enum Conv6Reduce { CONV6_REDUCE_NONE = 0, CONV6_REDUCE_SCALAR = 1, CONV6_REDUCE_FLOAT4 = 2, CONV6_REDUCE_BLOCKED = 3 };   // k_conv6_reduce<false | true>, k_conv6_reduce_blk
enum Conv6Valid { CONV6_FORM_OK = 0, CONV6_FORM_FORMAT_MISMATCH = 1 };
struct Conv6Form {
    Conv6Kernel kernel;
    int cfg;                        // tile configuration 0..3 (CONV6_TILE, conv6_device.h Cfg6)
    int ksplit;                     // workgroups per tile along K; > 1: partial sums into scratch, finished by the reduce kernel
    Conv6Reduce reduce;
    int nres;                       // k_conv6p: residual operands (its NRES)
    int vec4;                       // the convolution's epilogue may use aligned float4 accesses
    int tiles_h, tiles_w;
    int grid;                       // workgroups of the convolution launch
    Conv6Valid valid;               // anything but CONV6_FORM_OK: nothing may be launched
};

// pixel tile and workgroups per 64-row weight tile of each configuration (conv6_device.h checks these against Cfg6<CFG>)
struct Conv6Tile { int th, tw, mh; };
constexpr Conv6Tile CONV6_TILE[4] = {{16, 16, 1}, {16, 8, 1}, {8, 8, 1}, {16, 8, 2}};

// the epilogue may use aligned float4 accesses: interior rows start on a 16-byte boundary, and the residual operands are laid out as the output is
inline bool conv6_vec4_ok(int H, const Conv6Operand& out, const Conv6Operand& add1, const Conv6Operand& add2) {
    auto as_out = [&](const Conv6Operand& a) { return !a.on || (a.h0 == out.h0 && a.hp == out.hp); };
    return H % 4 == 0 && out.h0 % 4 == 0 && out.hp % 4 == 0 && as_out(add1) && as_out(add2);
}
// residual operands and output share one tensor format; BLOCKED needs whole channel blocks
inline bool conv6_formats_ok(int Cout, const Conv6Operand& out, const Conv6Operand& add1, const Conv6Operand& add2) {
    return !((add1.on && add1.blk != out.blk) || (add2.on && add2.blk != out.blk) || (out.blk && Cout % 8 != 0));
}

inline Conv6Form conv6_choose_form(const Conv6Shape& s, const Conv6Knobs& knobs, int ncu) {
    const int nchunk = (s.Cin + 15) / 16, n_ct = (s.Cout + 63) / 64;   // K chunks of 16 input channels; weight tiles of 64 output channels
    const Conv6Operand none;
    Conv6Form f = {CONV6_KERNEL_CONV6, 2, 1, CONV6_REDUCE_NONE, 0, 0, 0, 0, 0, CONV6_FORM_OK};
    if (!conv6_formats_ok(s.Cout, s.out, s.add1, s.add2)) { f.valid = CONV6_FORM_FORMAT_MISMATCH; return f; }
    // the largest pixel tile that still gives most CUs a workgroup (one workgroup per CU is the design point)
    auto ntiles = [&](int th, int tw) { return (long)n_ct * ((s.H + th - 1) / th) * ((s.W + tw - 1) / tw) * s.B; };
    // (tiles may overhang the image -- the kernel masks its stores -- as long as the padded area stays below 1.35 x the image)
    auto waste = [&](int th, int tw) { return (double)(((s.H + th - 1) / th) * th) * (((s.W + tw - 1) / tw) * tw) / ((double)s.H * s.W); };
    const long px = (long)s.H * s.W;
    const bool deep = px <= 32 * 32;                                // (by pixel count: the same choice at square levels, one rule for H != W)
    // 56 x 56 level (conv_midcfg): tile config of the split-K variant (0, 1), 2 = no split.  With blocked tensors the unsplit 64-pixel tiles (196
    // workgroups x 48 steps, no reduce launch) win: 696 vs 672 ADMM it/s on one box (round 2; with planar tensors split-K = 2 on
    // 128-pixel tiles + a reduce kernel was the faster form)
    // (3 = 128 pixels x 32 output channels, two workgroups per 64-row weight tile: half the weight bytes through LDS per MFMA of the
    //  64-pixel tile -- these levels' steps are bound by LDS traffic, 4 fragment reads per 3 MFMAs and a full weight step written per
    //  9 MFMAs of a wave: 743 -> 756 ADMM it/s with 3 / 3 / K over 4.  Measured and not kept on the way: one barrier per chunk instead
    //  of per step (six A buffers, whole chunks requested two ahead): 18.3 vs 18.2 us per launch, the barriers are not the bound.)
    // 28 x 28 level (conv_deepcfg, conv_deepks): tile config and largest K split.  Measured with blocked tensors on one box (ADMM it/s, two runs each):
    // 256-pixel tiles x 8 slices (the round-1 choice) 701.6 | x 4: 695 | 128-pixel x 4: 715 | x 2: 695 | 64-pixel x 2: 717.6 | x 1: 679;
    // then, on another box: 64-pixel x 2 (and 64-pixel unsplit at 56 x 56) 743 | configuration 3 at both levels, K over 2: 751.6 | over 4: 756
    const int level_cfg = deep ? knobs.conv_deepcfg : knobs.conv_midcfg;
    if (ntiles(16, 16) >= 160 && waste(16, 16) <= 1.35) f.cfg = 0;
    else if (ntiles(16, 8) >= 160 && waste(16, 8) <= 1.35) f.cfg = 1;
    else {
        // Small feature maps with many channels (the 28 x 28 x 512 level): a 64-pixel tile would re-read the layer's weights
        // once per tile (16 x 14 MB); instead keep the 256-pixel tile and split K over workgroups, then add the partial
        // outputs in slice order (deterministic) in a second, elementwise kernel.
        if (knobs.conv_splitk != 0 && nchunk >= 16) {
            // candidate: the 256-pixel tile (28 x 28 level) or the 128-pixel tile (56 x 56 level), K split so that about one
            // workgroup per CU results and every workgroup still walks >= 4 chunks
            const int cfg = level_cfg;
            const long nt = (cfg == 0) ? ntiles(16, 16) : (cfg == 1) ? ntiles(16, 8) : (cfg == 2) ? ntiles(8, 8) : 2 * ntiles(16, 8);
            int ksplit = 1;
            while ((deep || cfg < 2) && cfg >= 0 && ksplit * 2 * nt <= 256 && ksplit * 2 <= (deep ? knobs.conv_deepks : 8) && nchunk % (ksplit * 2) == 0 &&
                   nchunk / (ksplit * 2) >= 4)
                ksplit *= 2;
            if (ksplit > 1 && px <= 64 * 64) { f.cfg = (cfg > 3) ? 3 : cfg; f.ksplit = ksplit; }   // (a knob value above 3 counts as 3 here, as nt does)
        }
        // unsplit: configuration 3 where the level's knob names it and the layer fills whole 64-row weight tiles, else the 64-pixel tile
        if (f.ksplit == 1) f.cfg = (nchunk >= 16 && s.Cout % 64 == 0 && level_cfg == 3) ? 3 : 2;
    }
    const Conv6Tile t = CONV6_TILE[f.cfg];
    f.tiles_h = (s.H + t.th - 1) / t.th; f.tiles_w = (s.W + t.tw - 1) / t.tw;
    const long nt = (long)n_ct * f.tiles_h * f.tiles_w * s.B;
    // k_conv6p, the persistent form for slice batches (the two large tiles, unsplit): f16 scheme, whole 64-row weight tiles, an even number of
    // >= 4 chunks, BLOCKED tensors throughout, residual operands laid out exactly as the output (add2 only beside add1) ...
    auto as_out = [&](const Conv6Operand& a) { return !a.on || (a.blk && a.h0 == s.out.h0 && a.hp == s.out.hp && a.plane == s.out.plane); };
    const bool persistent = f.cfg < 2 && f.ksplit == 1 && knobs.conv_persist != 0 && s.sp6 == 2 && s.Cout % 64 == 0 && nchunk >= 4 && nchunk % 2 == 0 &&
                            !(s.add2.on && !s.add1.on) && s.in_blk && s.out.blk && as_out(s.add1) && as_out(s.add2) &&
                            nt > ncu;       // ... and more than one tile per CU: otherwise nothing to pipeline, k_conv6 is the same work
    if (persistent) {
        f.kernel = CONV6_KERNEL_CONV6P;
        f.nres = s.add2.on ? 2 : s.add1.on ? 1 : 0;
        f.vec4 = 1;
        f.grid = ncu;                                               // min(nt, ncu): one workgroup per CU
        return f;
    }
    if (f.ksplit > 1) {     // raw partial sums into planar scratch; the reduce kernel adds them and the residual operands, and applies the ReLU
        f.vec4 = conv6_vec4_ok(s.H, s.out, none, none) ? 1 : 0;
        f.reduce = s.out.blk ? CONV6_REDUCE_BLOCKED : conv6_vec4_ok(s.H, s.out, s.add1, s.add2) ? CONV6_REDUCE_FLOAT4 : CONV6_REDUCE_SCALAR;
    } else f.vec4 = conv6_vec4_ok(s.H, s.out, s.add1, s.add2) ? 1 : 0;
    f.grid = t.mh * n_ct * f.tiles_h * f.tiles_w * f.ksplit * s.B;
    return f;
}
#endif
