// conv6_form_test.cpp -- conv6_choose_form (csrc/conv6_form.h), the function conv6_launch asks for a 3x3 layer's launch form, on the host.
// Built and run by tests/test_conv_ref_host.py::test_launch_form_restatement_follows_the_library, which compares the answers with the
// tests' own restatement (tests/test_gpu_conv_layers.py launch_form).
//   stdin:  lines of  cin cout H W B blocked splitk persist midcfg deepcfg deepks [sp6 = 2]   (blocked: input AND output; no residual operand)
//   stdout: per line  cfg ksplit persistent reduce_kind vec4 grid                             (reduce_kind: 0 none, 1 scalar, 2 float4, 3 blocked)
// Tensors are laid out as qmri_set_denoiser allocates them (first interior row 32, row pitch a multiple of 32), on a chip of 256 CUs.
// Before it reads anything the program checks what the restatement does not model: residual operands and the format-mismatch code.
#include <cstdio>
#include "conv6_form.h"

static const int NCU = 256;

static Conv6Operand tensor(int H, int W, bool blk) {
    Conv6Operand t;
    t.on = true; t.blk = blk; t.h0 = 32; t.hp = ((t.h0 + H + 1 + 31) / 32) * 32; t.plane = (long)t.hp * (W + 2);
    return t;
}

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "conv6_form_test: line %d: %s is false\n", __LINE__, #cond); ++failed; } } while (0)

static int direct_checks() {
    int failed = 0;
    const Conv6Knobs knobs;
    const Conv6Operand t = tensor(64, 64, true), none;
    Conv6Shape s = {64, 64, 64, 64, 17, 2, true, t, none, none};        // 272 tiles of 16 x 16 on 256 CUs, blocked: the persistent form
    Conv6Form f = conv6_choose_form(s, knobs, NCU);
    EXPECT(f.valid == CONV6_FORM_OK && f.kernel == CONV6_KERNEL_CONV6P && f.cfg == 0 && f.nres == 0 && f.vec4 == 1 && f.grid == NCU);
    s.add1 = t;
    f = conv6_choose_form(s, knobs, NCU);
    EXPECT(f.kernel == CONV6_KERNEL_CONV6P && f.nres == 1);
    s.add2 = t;
    f = conv6_choose_form(s, knobs, NCU);
    EXPECT(f.kernel == CONV6_KERNEL_CONV6P && f.nres == 2);
    s.add1 = none;                                                      // add2 without add1
    f = conv6_choose_form(s, knobs, NCU);
    EXPECT(f.valid == CONV6_FORM_OK && f.kernel == CONV6_KERNEL_CONV6 && f.cfg == 0 && f.vec4 == 1 && f.grid == 272);
    s.add1 = t; s.add2 = none;
    s.add1.hp += 32; s.add1.plane = (long)s.add1.hp * 66;               // a residual operand with another row pitch
    f = conv6_choose_form(s, knobs, NCU);
    EXPECT(f.valid == CONV6_FORM_OK && f.kernel == CONV6_KERNEL_CONV6 && f.vec4 == 0 && f.grid == 272);
    EXPECT(!conv6_vec4_ok(64, t, s.add1, none) && conv6_vec4_ok(64, t, t, t) && !conv6_vec4_ok(62, t, none, none));
    s.add1 = tensor(64, 64, false);                                     // a planar residual operand beside a blocked output
    EXPECT(conv6_choose_form(s, knobs, NCU).valid == CONV6_FORM_FORMAT_MISMATCH);
    s.add1 = none; s.add2 = tensor(64, 64, false);
    EXPECT(conv6_choose_form(s, knobs, NCU).valid == CONV6_FORM_FORMAT_MISMATCH);
    s.add2 = none; s.Cout = 60;                                         // blocked output without whole channel blocks
    EXPECT(conv6_choose_form(s, knobs, NCU).valid == CONV6_FORM_FORMAT_MISMATCH);
    s.out.blk = false; s.in_blk = false;
    EXPECT(conv6_choose_form(s, knobs, NCU).valid == CONV6_FORM_OK);
    // split-K: the convolution's own vec4 ignores the residual operands (they belong to the reduce kernel), whose kind follows them
    Conv6Shape d = {256, 64, 16, 16, 1, 2, false, tensor(16, 16, false), none, none};
    f = conv6_choose_form(d, knobs, NCU);
    EXPECT(f.cfg == 3 && f.ksplit == 4 && f.reduce == CONV6_REDUCE_FLOAT4 && f.vec4 == 1 && f.grid == 2 * 1 * 1 * 2 * 4);
    d.add1 = tensor(16, 16, false); d.add1.h0 = 1;
    f = conv6_choose_form(d, knobs, NCU);
    EXPECT(f.cfg == 3 && f.ksplit == 4 && f.reduce == CONV6_REDUCE_SCALAR && f.vec4 == 1);
    return failed;
}

int main() {
    if (direct_checks()) return 1;
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int cin, cout, H, W, B, blocked, sp6 = 2;
        Conv6Knobs k;
        const int n = sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d %d", &cin, &cout, &H, &W, &B, &blocked, &k.conv_splitk, &k.conv_persist, &k.conv_midcfg,
                             &k.conv_deepcfg, &k.conv_deepks, &sp6);
        if (n < 11) { fprintf(stderr, "conv6_form_test: malformed line: %s", line); return 2; }
        const Conv6Shape s = {cin, cout, H, W, B, sp6, blocked != 0, tensor(H, W, blocked != 0), Conv6Operand(), Conv6Operand()};
        const Conv6Form f = conv6_choose_form(s, k, NCU);
        if (f.valid != CONV6_FORM_OK) { fprintf(stderr, "conv6_form_test: validity code %d for: %s", (int)f.valid, line); return 3; }
        printf("%d %d %d %d %d %d\n", f.cfg, f.ksplit, f.kernel == CONV6_KERNEL_CONV6P ? 1 : 0, (int)f.reduce, f.vec4, f.grid);
    }
    return 0;
}
