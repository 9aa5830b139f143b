"""The side outputs' shared path (bvcf_outputs.cpp) without a device, in a stand-alone program under the address and
undefined-behaviour sanitizers (outputs_check.cpp has the list): the run tables carried over reservation regrows and summed
over workers against direct 128-bit addition; open_outputs and finish_outputs after a failed run and after a successful one
-- what is in the files, and that no descriptor stays open."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bystro-vcf_amd", "csrc")
LIBDIR = os.path.join(ROOT, "bystro-vcf_amd")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


def test_outputs_path_alone_under_sanitizers(tmp_path):
    if os.path.exists("/dev/kfd"):
        pytest.skip("GPU present: sanitized programs run on the build machine")
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "outputs_check")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-result", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", "outputs_check.cpp"), "-o", exe, "-L", LIBDIR, "-lbvcf", "-Wl,-rpath," + LIBDIR], timeout=180)
    work = tmp_path / "files"
    work.mkdir()
    p = subprocess.run([exe, str(work)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.endswith("outputs ok\n"), out[-3000:]
    assert "ERROR" not in out and "runtime error" not in out, out[-3000:]
    # (what the successful pass wrote: the headers and the summed tables of the program's three samples)
    assert (work / "stats").read_text().startswith("sample\thet\thom\t") and (work / "stats").read_text().count("\n") == 4
    assert (work / "pairs").read_text().count("\n") == 4 and (work / "scores").read_text().startswith("sample\tmatched\tcalled\tdosageSum\ta_SUM\ta_AVG\tb_SUM")
    assert (work / "site.report").read_text().split("\n")[1] == "kept\t12" and (work / "region.report").read_text().split("\n")[4] == "dropped\t9"
