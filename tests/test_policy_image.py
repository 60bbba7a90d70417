"""The packed float32 image of csrc/policy.h on the host: tests/native/policy_image_host.cpp, built together with csrc/policy.cpp
by the compiler line csrc/Makefile uses for policy.cpp, packs 71 -> 96 -> 40 -> 6 and 3 -> 1 with gs_policy_pack_f32, checks every
slot against the layout's description (padding zero), unpacks every layer with gs_policy_unpack_f32 back to the exact float32 values
and compares each transposed image with the pack of W^T.  No device."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grid_fed_rl_gym_amd", "csrc")


def test_pack_unpack_round_trip_and_transposed_image(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "policy_image_host"
    # (csrc/Makefile, build/policy.o: $(HIPCC) -O2 -std=c++17 -fPIC -Wall -x c++)
    subprocess.run([hipcc, "-O2", "-std=c++17", "-fPIC", "-Wall", "-Werror", "-I", CSRC, "-x", "c++", os.path.join(CSRC, "policy.cpp"),
                    os.path.join(ROOT, "tests", "native", "policy_image_host.cpp"), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["dims 71 96 40 6: ok", "dims 3 1: ok"], r.stdout + r.stderr
