"""CPU: the memory owners of the library (csrc/dev_mem.h) where no GPU test can reach them -- with no device every allocation fails -- and the
diagnostic hook that counts their allocations."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc")


def test_hook_declared_exported_and_zero_without_allocations():
    from qmri_pnp_recon_poc_amd import _lib
    header = open(os.path.join(ROOT, "include", "qmri.h")).read()
    assert re.search(r"\bint\s+qmri_debug_mem_stats\s*\(qmri_mem_stats\* out\)", header)
    assert "qmri_debug_mem_stats" in _lib.SYMBOLS
    L = _lib.lib()
    assert C.sizeof(_lib.MemStats) == 48
    assert L.qmri_debug_mem_stats(None) == -1
    s = _lib.MemStats(*([-1] * 6))
    assert L.qmri_debug_mem_stats(C.byref(s)) == 0
    assert (s.dev_live, s.dev_bytes, s.pinned_live, s.pinned_bytes) == (0, 0, 0, 0)      # (no context has been made in this process)


def test_one_file_calls_the_allocator():
    """The grep of the refactor: outside dev_mem.h nothing under csrc/ or mex/ names the HIP allocator, and no hand-kept list of pointers to free is left."""
    pat = re.compile(r"hipMalloc|hipFree|hipHostMalloc|hipHostFree|void\*\s+ptrs\[\]")
    hits = []
    for d in (CSRC, os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "mex")):
        for f in sorted(os.listdir(d)):
            if f.endswith((".cpp", ".hip", ".h")) and f != "dev_mem.h":
                for n, line in enumerate(open(os.path.join(d, f), errors="replace"), 1):
                    if pat.search(line):
                        hits.append(f"{f}:{n}: {line.strip()[:100]}")
    assert not hits, hits


def test_failure_contract_under_address_and_ub_sanitizer():
    """`make asan-host` builds tests/cpp/host_asan_devmem.cpp against the host-only sanitised library: a failed ensure / alloc leaves the owner
    empty with QMRI_ERR_NOMEM and a message, reset and move are harmless on empty and moved-from owners, a pool frees only what it got, the plans
    are replaced by fresh values, and the counters stay at zero throughout."""
    subprocess.run(["make", "-C", CSRC, "-s", "-j4", "asan-host"], check=True)
    base = "/opt/rocm/lib/llvm/lib/clang"
    rt_dirs = [d for d in sorted(os.listdir(base)) if os.path.isdir(os.path.join(base, d, "lib", "linux"))]
    if not rt_dirs:
        pytest.skip("clang sanitizer runtime not found")
    rt = os.path.join(base, rt_dirs[-1], "lib", "linux")
    env = dict(os.environ, LD_LIBRARY_PATH=rt + ":" + os.environ.get("LD_LIBRARY_PATH", ""),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77", UBSAN_OPTIONS="halt_on_error=1:exitcode=78:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_build_asan", "host_asan_devmem")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST_ASAN_DEVMEM_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
