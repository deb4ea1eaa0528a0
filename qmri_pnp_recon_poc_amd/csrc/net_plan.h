// net_plan.h -- the denoiser's layer program: which layers a qmri_net_desc has, in the order of the weight blob, which tensor each one reads,
// writes and adds, how many channels every tensor is allocated with, and which runs of layers the resident-tile launch may be offered
// (k_conv6r, conv6r_kernels.hip).  ONE builder, net_plan_build(), for both architectures.  api_net.cpp counts the weights, plans the layers,
// allocates the tensors and walks the forward pass from its result; nothing else states the layer order.  No HIP, no context: plain C++17, so that
// tests/cpp/net_plan_test.cpp prints the program the library runs and tests/test_net_plan_host.py executes it in fp64 on a machine without a GPU.
#ifndef QMRI_NET_PLAN_H            // (a guard, not #pragma once: the header is also compiled on its own)
#define QMRI_NET_PLAN_H

#include <algorithm>
#include <cstddef>
#include <vector>

#include "../../include/qmri.h"

enum ConvKind { CONV_3X3 = 0, CONV_DOWN = 1, CONV_UP = 2, CONV_3X3N = 3 };   // 3X3N: 3x3 with 32-channel chunks (Cin <= 64)
constexpr int CONV_CHUNK[4] = {64, 32, 128, 32};                    // input channels per chunk, by ConvKind (conv_kernels.hip checks these against Geo<KIND>::CC)
inline ConvKind conv_narrow(ConvKind kind, int Cin) { return (kind == CONV_3X3 && Cin <= 64) ? CONV_3X3N : kind; }   // narrow 3x3 layers: 32-channel chunks
// channels a layer reads of its input tensor: whole chunks, and >= 2 of them (the tile pipeline needs a barrier between a tile's first step and its last)
inline int conv_cin_pad(ConvKind kind, int Cin) {
    const int CC = CONV_CHUNK[conv_narrow(kind, Cin)];
    return std::max(2 * CC, ((Cin + CC - 1) / CC) * CC);
}

// The tensors of a forward pass (NetPlan::ten, qmri_internal.h).  Per UNet level l the skip tensor x and two work tensors a, t, level after level
// (the order they are allocated in); SEQ_CONV ping-pongs between a[0] and t[0].
enum NetTensor { NT_NONE = -1, NT_X0 = 0, NT_A0 = 1, NT_T0 = 2, /* level l: + 3 l */ NT_IN32 = 12, NT_OUT32 = 13, NT_COUNT = 14 };
inline NetTensor nt_x(int l) { return (NetTensor)(NT_X0 + 3 * l); }
inline NetTensor nt_a(int l) { return (NetTensor)(NT_A0 + 3 * l); }
inline NetTensor nt_t(int l) { return (NetTensor)(NT_T0 + 3 * l); }
inline bool nt_interior(NetTensor id) { return id >= 0 && id < NT_IN32; }   // everything between the first layer's input and the last layer's output
inline int nt_level(NetTensor id) { return nt_interior(id) ? id / 3 : 0; }  // spatial size (H >> level) x (W >> level)

// one layer: out = conv(in) [+ add1] [+ add2] [ReLU]
struct NetStep {
    ConvKind kind;                  // as the architecture names it (CONV_3X3 | CONV_DOWN | CONV_UP): BEFORE conv_plan_layer renames narrow 3x3 layers
    int Cin, Cout;
    size_t w_off;                   // first weight in the flat blob (floats)
    int level;                      // level of `in` (CONV_DOWN writes level + 1, CONV_UP level - 1)
    NetTensor in, out, add1, add2;
    int relu_out;
};
// a run of steps that may go out as ONE resident-tile launch (Conv6rRun, qmri_internal.h): steps first .. first + count - 1 = [head] 2 nb ResBlock layers
// [tail | down]; step indices, -1: not part of the run
constexpr int NET_RUN_MAXL = 10;    // layers per resident-tile launch (conv6r_kernels.hip R_MAXL)
struct NetRun {
    int first, count;
    int head, res, nres, tail, down;
    NetTensor src, cur, skip, head_in, tail_out, down_out;
};
// knobs res_head / res_tail / res_down (qmri_internal.h): a run with the head / tail / down-sampling convolution inside is offered only with its knob on
inline bool net_run_allowed(const NetRun& r, bool res_head, bool res_tail, bool res_down) {
    return (r.head < 0 || res_head) && (r.tail < 0 || res_tail) && (r.down < 0 || res_down);
}

struct NetProgram {
    std::vector<NetStep> steps;     // blob order = execution order
    std::vector<NetRun> runs;       // ascending `first`; runs that start at the same step in order of preference (the first one taken skips the others)
    size_t nparams = 0;             // floats of the weight blob
    int chan[NT_COUNT] = {};        // channels of every tensor; 0: the architecture has no such tensor
    int cal[NT_COUNT] = {};         // channels it is allocated with
    bool blk_ok = true;             // channel counts allow BLOCKED interior tensors (PTensor::blk): every used one's and every allocation's a multiple of 8
};

inline NetProgram net_plan_build(const qmri_net_desc& d) {
    NetProgram P;
    const int nb = d.nb;
    auto step = [&](ConvKind kind, int cin, int cout, NetTensor in, NetTensor out, NetTensor add1 = NT_NONE, NetTensor add2 = NT_NONE, int relu = 0) {
        P.steps.push_back({kind, cin, cout, P.nparams, nt_level(in), in, out, add1, add2, relu});
        P.nparams += (size_t)cin * cout * (kind == CONV_3X3 ? 9 : 4);
    };
    if (d.arch == QMRI_ARCH_UNETRES) {                              // UNetRes.forward, network_unet.py:106-117; layer order of state_dict(), :68-117
        const int32_t* nc = d.nc;
        for (int l = 0; l < 4; ++l) P.chan[nt_x(l)] = P.chan[nt_a(l)] = P.chan[nt_t(l)] = nc[l];
        // nb ResBlocks: cur <- cur + conv(relu(conv(cur)))  (basicblock.py:211-223).  `src` is the block input of the first ResBlock (may be a skip
        // tensor that must stay intact); results land in a[l]; `skip` is added by the last conv.  Returns the first step's index.
        auto resblocks = [&](int l, NetTensor src, NetTensor skip) {
            const int first = (int)P.steps.size();
            NetTensor in = src;
            for (int b = 0; b < nb; ++b) {
                step(CONV_3X3, nc[l], nc[l], in, nt_t(l), NT_NONE, NT_NONE, 1);
                step(CONV_3X3, nc[l], nc[l], nt_t(l), nt_a(l), in, (b == nb - 1) ? skip : NT_NONE);
                in = nt_a(l);
            }
            return first;
        };
        // the full-resolution level's candidates: the ResBlock layers at `res` with the steps before (head) / behind them (tail, down) that are named
        auto run = [&](int res, bool head, bool tail, bool down, NetTensor src, NetTensor skip) {
            const int count = 2 * nb + head + tail + down, behind = res + 2 * nb;
            if (nb < 1 || count > NET_RUN_MAXL) return;
            P.runs.push_back({res - head, count, head ? res - 1 : -1, res, 2 * nb, tail ? behind : -1, down ? behind : -1, src, NT_A0, skip,
                              head ? NT_IN32 : NT_NONE, tail ? NT_OUT32 : NT_NONE, down ? nt_x(1) : NT_NONE});
        };
        step(CONV_3X3, d.in_nc, nc[0], NT_IN32, NT_X0);                                                      // x1 = m_head(x0)
        for (int l = 0; l < 3; ++l) {                                                                        // x_{l+2} = m_down_{l+1}(x_{l+1})
            const int res = resblocks(l, nt_x(l), NT_NONE);
            step(CONV_DOWN, nc[l], nc[l + 1], nt_a(l), nt_x(l + 1));
            if (l == 0) { run(res, true, false, true, NT_X0, NT_NONE); run(res, true, false, false, NT_X0, NT_NONE); run(res, false, false, false, NT_X0, NT_NONE); }
        }
        resblocks(3, nt_x(3), nt_x(3));                                                                      // m_body(x4) + x4
        for (int l = 3; l > 0; --l) {                                                                        // m_up_l(x + x_{l+1})
            step(CONV_UP, nc[l], nc[l - 1], nt_a(l), nt_a(l - 1));                                           // transposed conv
            const int res = resblocks(l - 1, nt_a(l - 1), nt_x(l - 1));                                      // (in place: the first ResBlock's add1 is its in)
            if (l == 1) { run(res, false, true, false, NT_A0, NT_X0); run(res, false, false, false, NT_A0, NT_X0); }
        }
        step(CONV_3X3, nc[0], d.out_nc, NT_A0, NT_OUT32);                                                    // m_tail(x + x1)
    } else if (d.arch == QMRI_ARCH_SEQ_CONV) {                      // nb layers conv3x3 (+ ReLU but behind the last), width nc[0], between a[0] and t[0]
        const int width = d.nc[0];
        P.chan[NT_A0] = P.chan[NT_T0] = width;
        for (int l = 0; l < nb; ++l) {
            const bool first = l == 0, last = l == nb - 1;
            step(CONV_3X3, first ? d.in_nc : width, last ? d.out_nc : width, first ? NT_IN32 : (l & 1) ? NT_A0 : NT_T0, last ? NT_OUT32 : (l & 1) ? NT_T0 : NT_A0,
                 NT_NONE, NT_NONE, !last);
        }
    } else return P;
    P.chan[NT_IN32] = d.in_nc; P.chan[NT_OUT32] = d.out_nc;
    // Channels allocated: the largest padded Cin of any layer that reads the tensor -- for the interior tensors of any layer that reads a tensor of
    // their level, so that a level's three tensors stay interchangeable -- and never below the tensor's own channels.  (An interior tensor of a level
    // nobody reads, the one-layer SEQ_CONV's pair, gets what a 3x3 layer of its own width would read.)
    int level_pad[4] = {0, 0, 0, 0}, pad[NT_COUNT] = {};
    for (const NetStep& s : P.steps) {
        int& m = nt_interior(s.in) ? level_pad[s.level] : pad[s.in];
        m = std::max(m, conv_cin_pad(s.kind, s.Cin));
        for (NetTensor t : {s.in, s.out}) if (nt_interior(t) && P.chan[t] % 8) P.blk_ok = false;
    }
    for (int id = 0; id < NT_COUNT; ++id) {
        const NetTensor t = (NetTensor)id;
        if (nt_interior(t) && P.chan[t]) pad[id] = level_pad[nt_level(t)] ? level_pad[nt_level(t)] : conv_cin_pad(CONV_3X3, P.chan[t]);
        P.cal[id] = std::max(P.chan[id], pad[id]);
        if (nt_interior(t) && P.cal[id] % 8) P.blk_ok = false;
    }
    return P;
}

inline size_t net_plan_nparams(const qmri_net_desc& d) { return net_plan_build(d).nparams; }
#endif
