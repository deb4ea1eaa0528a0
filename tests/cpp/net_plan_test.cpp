// Prints the denoiser's layer program (csrc/net_plan.h) for every descriptor line on stdin:
//   arch in_nc out_nc nc0 nc1 nc2 nc3 nb res_head res_tail res_down
// one "step" line per layer, one "tensor" line per tensor the architecture has, the totals, and one "run" line per resident-run candidate the
// three knobs leave.  tests/test_net_plan_host.py compares the lines with the tests' own statements of the architectures and executes them in fp64.
// Plain C++17, built with the address and undefined-behaviour sanitizers; no GPU, no HIP.
#include <cstdio>
#include <string>

#include "net_plan.h"

static std::string name(NetTensor t) {
    if (t == NT_NONE) return "none";
    if (t == NT_IN32) return "in32";
    if (t == NT_OUT32) return "out32";
    return std::string(1, "xat"[t % 3]) + std::to_string(nt_level(t));
}

int main() {
    qmri_net_desc d{};
    int arch, in_nc, out_nc, nc[4], nb, knob[3], nets = 0;
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d", &arch, &in_nc, &out_nc, &nc[0], &nc[1], &nc[2], &nc[3], &nb, &knob[0], &knob[1], &knob[2]) == 11) {
        d.arch = arch; d.in_nc = in_nc; d.out_nc = out_nc; d.nb = nb;
        for (int l = 0; l < 4; ++l) d.nc[l] = nc[l];
        const NetProgram P = net_plan_build(d);
        if (P.nparams != net_plan_nparams(d)) { std::fprintf(stderr, "net_plan_nparams differs from the program's sum\n"); return 1; }
        std::printf("net %d\n", nets++);
        for (size_t i = 0; i < P.steps.size(); ++i) {
            const NetStep& s = P.steps[i];
            std::printf("step %zu kind=%d cin=%d cout=%d w_off=%zu level=%d in=%s out=%s add1=%s add2=%s relu=%d\n", i, (int)s.kind, s.Cin, s.Cout, s.w_off, s.level,
                        name(s.in).c_str(), name(s.out).c_str(), name(s.add1).c_str(), name(s.add2).c_str(), s.relu_out);
        }
        for (int id = 0; id < NT_COUNT; ++id)
            if (P.chan[id]) std::printf("tensor %s chan=%d cal=%d\n", name((NetTensor)id).c_str(), P.chan[id], P.cal[id]);
        std::printf("total nparams=%zu blk_ok=%d\n", P.nparams, P.blk_ok ? 1 : 0);
        for (const NetRun& r : P.runs) {
            if (!net_run_allowed(r, knob[0] != 0, knob[1] != 0, knob[2] != 0)) continue;
            std::printf("run first=%d count=%d head=%d res=%d nres=%d tail=%d down=%d src=%s cur=%s skip=%s head_in=%s tail_out=%s down_out=%s\n", r.first, r.count, r.head,
                        r.res, r.nres, r.tail, r.down, name(r.src).c_str(), name(r.cur).c_str(), name(r.skip).c_str(), name(r.head_in).c_str(),
                        name(r.tail_out).c_str(), name(r.down_out).c_str());
        }
    }
    return nets ? 0 : 1;
}
