"""CPU: the host planning of a gridded operator (csrc/op_plan.h) -- the mask builders, the k-sorted sample list, the work units of the k-space LSQR
and the DIRECT solver's tables -- through the stand-alone program tests/cpp/op_plan_test.cpp, built with the address and undefined-behaviour
sanitizers.  The program checks, case by case, what holds whatever the planner's thresholds are; this file holds what the thresholds give."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# case -> (status, unit shape, units, n, tried, digest of sgrp / es / grp / units).  Recorded from the planner as it stood inside qmri_set_operator
# before it moved into op_plan.h (its lambda and selection code copied verbatim into a scratch program and run on these masks), NOT from
# ks_plan_units: a changed threshold (250, the 320 above which a larger shape is tried, 8 samples per k, the step of 8, the order of the larger shapes,
# the re-cut) changes a line here.  Not reached by any mask found so far: the 320 that ends the attempts of one cut early (no case has a first
# attempt inside 301 .. 345 units that later attempts would shrink).
# status 1 = "a k location is sampled n times; at most `tried` ...", 2 = "V does not fit".  s = 10, 256 CUs, every shape's V fits unless the name says otherwise.
EXPECTED = {
    "spiral32_S400_T24":            (0, 0, 240, 0, 0, "e8803d04f63d17e1"),      # dense, the first attempt
    "spiral32_S400_T24/v_too_large": (2, 0, 240, 0, 0, "0000000000000000"),     # lds_fits[0] = false
    "spiral32_S57_T9":              (0, 3, 128, 0, 0, "70c9a62fed8e5aab"),      # sparse
    "full16_T8_last255":            (0, 3, 255, 0, 0, "b0ed0266d210a3a3"),      # 7.996 samples per sampled k: sparse
    "full16_T8":                    (0, 0, 256, 0, 0, "aa75fbc94b196670"),      # 8: dense
    "spiral224_S771_T200/B1":       (0, 0, 250, 0, 0, "2edc5688c861cf75"),      # the headline operator: 263 -> 250 in three attempts
    "spiral224_S771_T200/B15":      (0, 0, 250, 0, 0, "2edc5688c861cf75"),
    "epi128_5th_T100":              (0, 0, 316, 0, 0, "a1c001deebf8230a"),      # the 251..320 band: eight attempts, no upgrade
    "epi160_5th_T9/B1":             (0, 1, 248, 0, 0, "ae1f76b9b9c4668c"),      # 400 units of shape 3 -> shape 1
    "epi160_5th_T9/B4_off":         (0, 3, 400, 0, 0, "c1a0aa53315873e3"),      # slice batches without the one-launch iteration keep the small shape
    "epi160_5th_T9/ncu64":          (0, 3, 400, 0, 0, "c1a0aa53315873e3"),      # upgrade refused (248 > 64 CUs), re-cut
    "epi160_5th_T9/no1":            (0, 3, 400, 0, 0, "c1a0aa53315873e3"),      # lds_fits[1] = false: shape 2 gives 400 > 256, back to the base
    "epi160_5th_T9/no12":           (0, 3, 400, 0, 0, "c1a0aa53315873e3"),
    "epi160_5th_T9/s6":             (0, 3, 400, 0, 0, "c1a0aa53315873e3"),      # s != 10: no upgrade
    "epi128_5th_T30/B1":            (0, 1, 247, 0, 0, "97401eb082c01efb"),
    "epi128_5th_T30/no1":           (0, 2, 256, 0, 0, "3d40f842a83df10f"),      # lds_fits[1] = false: the sparse mask on shape 2
    "epi224_65th_T200/B1":          (0, 1, 245, 0, 0, "dcae0350da7e79bc"),
    "epi256_65th_T200/B1":          (0, 1, 256, 0, 0, "d4b98afbeeb89fd4"),      # eight attempts of the upgrade
    "full32_T300/B1":               (0, 2, 205, 0, 0, "d2f6559980759e8b"),      # 342 units of shape 0 -> shape 2
    "full32_T300/B4_off":           (0, 0, 342, 0, 0, "28eb22c4597b2c05"),
    "full32_T300/ncu100":           (0, 0, 342, 0, 0, "28eb22c4597b2c05"),
    "cut0_spiral224_S771_T1000/B1": (0, 2, 256, 0, 0, "fc17c03c3e34bd22"),      # 632 units of shape 0 -> 256 of shape 2 (not <= 250)
    "busy16_T300":                  (0, 0, 65, 0, 0, "23ba5af92b2288db"),       # sparse on average, k = 0 in 300 frames: shape 3 refuses, the dense one takes it
    "busy16_T1100/B1":              (0, 2, 38, 0, 0, "3a0b317f5e43c505"),       # shapes 3, 0 and 1 refuse
    "busy16_T1100/B4_off":          (1, -1, 0, 1100, 1024, "0000000000000000"),
    "k0_T2600/B1":                  (1, -1, 0, 2600, 2560, "0000000000000000"),
    # The 32-sided masks that tests/test_gpu_gridded_sweep.py runs on the device (beside spiral32_*, full32_T300/B1 above and the epi masks), so that
    # the unit shape each of those cases reaches is pinned here: the GPU test cannot read it.  Unlike the lines above, these digests were recorded from
    # ks_plan_units as it stands in op_plan.h; what they pin is the shape and the unit count.
    "busy32_T300":                  (0, 0, 148, 0, 0, "bcbef29541514020"),      # sparse on average, k = 0 in 300 frames: shape 3 refuses, shape 0 takes it
    "busy32_T1100":                 (0, 2, 104, 0, 0, "c5d7a6d5b62bde4d"),      # only shape 2 holds the 1100 samples of k = 0 (35 scatter groups of one slot)
    "full32_T8":                    (0, 0, 205, 0, 0, "93937807f99cc39f"),      # 8 samples per k: dense
    "full32_T8_last1023":           (0, 3, 205, 0, 0, "7f9aeaa1e2a28572"),      # 7.999: sparse
    "single_sample32":              (0, 3, 1, 0, 0, "e35c1f865048853b"),        # m = 1: one unit of one slot
}


def test_operator_plan_on_the_host_under_sanitizers(tmp_path):
    exe = tmp_path / "op_plan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "op_plan_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    got = {}
    for ln in r.stdout.splitlines():
        name, *fields = ln.split()
        kv = dict(f.split("=") for f in fields)
        if name != "direct_inverse":
            got[name] = (int(kv["status"]), int(kv["caps"]), int(kv["units"]), int(kv["n"]), int(kv["tried"]), kv["digest"])
    assert "direct_inverse" in r.stdout
    assert sorted(got) == sorted(EXPECTED)
    wrong = {k: (got[k], EXPECTED[k]) for k in EXPECTED if got[k] != EXPECTED[k]}
    assert not wrong, wrong


def test_op_plan_header_stands_alone():
    """op_plan.h is plain C++17: it compiles on its own, without HIP and without the library's other headers."""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++",
                        os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc", "op_plan.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
