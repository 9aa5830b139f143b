"""bvcf_devmem.h, the owners of the ctx's device and pinned buffers, streams and events: a stand-alone host program
(tests/devmem_check.cpp) under the address and undefined-behaviour sanitizers.  Without a GPU every allocation of the HIP
runtime fails, which is the path the GPU tests never reach; the same program over malloc-backed stand-ins of the runtime's
calls checks that nothing is freed twice or lost."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bystro-vcf_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ROCM = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))
ROCM_LIB = os.path.join(ROCM, "lib")


def _build_and_run(tmp_path, name, extra):
    if os.path.exists("/dev/kfd"):
        pytest.skip("GPU present: the sanitized program must not open it")
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / name)
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", os.path.join(ROCM, "include"),
                           os.path.join(ROOT, "tests", "devmem_check.cpp"), "-o", exe] + extra, timeout=120)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = p.stdout.decode()
    assert p.returncode == 0 and "devmem ok" in out, out
    assert "ERROR" not in out and "runtime error" not in out, out
    return out


def test_failed_allocations_leave_the_owners_empty(tmp_path):
    out = _build_and_run(tmp_path, "devmem_check", ["-L", ROCM_LIB, "-lamdhip64", "-Wl,-rpath," + ROCM_LIB])
    assert "device: alloc -> " in out and "pinned: alloc -> " in out
    assert "alloc -> 0 " not in out


def test_owners_free_once_and_lose_nothing(tmp_path):
    """... and the test mode (BVCF_POISON): the fills, the guards' reports by side, offset and allocation site, damage seen
    only at reset(), the registry under moves and failed allocations, and the off mode asking for exactly today's bytes"""
    out = _build_and_run(tmp_path, "devmem_check_stand_ins", ["-DDEVMEM_STAND_INS"])
    assert "poison ok" in out
