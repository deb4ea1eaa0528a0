"""Host check (no GPU) of the FFT codelets and per-axis plans that the operator's grid sizes use."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fft_plans_on_host(tmp_path):
    exe = tmp_path / "fft_plans_test"
    subprocess.run(["g++", "-O2", "-I", os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "fft_plans_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    for name in ("dft3", "dft5", "dft6", "dft10", "dft12", "plan8x12", "plan16x7", "plan16x10", "plan16x12", "plan16x16 inv"):
        assert name in r.stdout
