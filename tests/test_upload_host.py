"""The host half of rpt_upload_scene (csrc/host_upload.h; CPU only) under the address and undefined-behaviour sanitizers: every error
case of every scene class with its code and message, the class map against its definition, large and mesh images read back through
their bound pointers, the same bytes from the same input (tests/upload_harness.cpp).  The headers include hip_runtime.h, so hipcc
compiles them host-only; the binary has no device code and does not link the HIP runtime."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_upload_host_half_under_sanitizers(tmp_path):
    exe = str(tmp_path / "upload_harness")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    # (-Xarch_host: the sanitizers instrument host code only; the file has no device code anyway)
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wl,--as-needed", os.path.join(ROOT, "tests", "upload_harness.cpp"),
                    "-o", exe], check=True)
    dyn = subprocess.run(["readelf", "-d", exe], check=True, capture_output=True, text=True).stdout
    assert "NEEDED" in dyn and "libamdhip64" not in dyn, dyn
    syms = subprocess.run(["nm", exe], check=True, capture_output=True, text=True).stdout
    assert "__asan_report" in syms and "__ubsan_handle" in syms, "the harness is not instrumented"
    env = {k: v for k, v in os.environ.items() if not k.startswith("RPT_")}
    modes = ["errors", "classmap", "readback", "same"]
    r = subprocess.run([exe] + modes, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["%s OK" % m for m in modes], r.stdout
    r = subprocess.run([exe, "huge"], capture_output=True, text=True, timeout=600, env=dict(env, RPT_NO_GRID="1"))
    assert r.returncode == 0 and r.stdout.strip() == "huge OK", r.stdout + r.stderr
