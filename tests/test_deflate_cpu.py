"""--compressOutput / bvcf_bgzf_deflate_device / bvcf_config.out_bgzf: what can be checked without a device."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bystro-vcf_amd", "bystro-vcf")


@pytest.fixture(scope="module")
def bv():
    import bystro_vcf_amd as b
    return b


def _cli(args):
    if not os.path.exists(EXE):
        pytest.skip("CLI not built")
    return subprocess.run([EXE] + args, input=b"", capture_output=True, timeout=60)


@pytest.mark.parametrize("args", [["--compressOutput", "zip"], ["--compressOutput=gzip"], ["-compressOutput", ""]])
def test_compress_output_rejects_unknown_values(args):
    p = _cli(args)
    val = args[-1].split("=")[-1] if "=" in args[-1] else args[-1]
    assert p.returncode == 2
    assert ('invalid value "%s" for flag -compressOutput' % val).encode() in p.stderr


def test_compress_output_needs_a_value():
    p = _cli(["--compressOutput"])
    assert p.returncode == 2 and b"flag needs an argument: -compressOutput" in p.stderr


def test_compress_output_none_is_accepted_before_any_work():
    # an accepted value goes on to the run: the empty stdin is then what fails ("EOF"), not the flag
    for v in ("none", "bgzf"):
        p = _cli(["--compressOutput", v])
        assert b"flag provided but not defined" not in p.stderr and b"invalid value" not in p.stderr


def test_deflate_without_device_is_nodev(bv):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cap = bv.bgzf_bound(100)
    buf = C.create_string_buffer(cap)
    n = C.c_size_t(7)
    assert bv.lib.bvcf_bgzf_deflate_device(0, b"x" * 100, 100, 1, buf, cap, C.byref(n)) == bv.E_NODEV
    with pytest.raises(bv.BvcfError) as ei:
        bv.bgzf_deflate_device(b"hello")
    assert ei.value.rc == bv.E_NODEV


def test_bound_matches_header(bv):
    # 18 + 5 + 65280 + 8 bytes per piece (one stored member), plus the EOF block
    assert bv.bgzf_bound(0) == 28
    assert bv.bgzf_bound(1) == bv.bgzf_bound(65280) == 65311 + 28
    assert bv.bgzf_bound(65281) == 2 * 65311 + 28
    assert len(bv.BGZF_EOF) == 28


def test_config_out_bgzf_offset_matches_header(bv, tmp_path):
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bvcf.h"\n'
                   "int main(){printf(\"%zu %zu %zu %zu\\n\", offsetof(bvcf_config, no_out), offsetof(bvcf_config, out_bgzf),"
                   "offsetof(bvcf_config, reserved3), sizeof(bvcf_config));"
                   "bvcf_config c; bvcf_config_defaults(&c); printf(\"%d\\n\", (int)c.out_bgzf); return 0;}\n")
    exe = tmp_path / "off"
    subprocess.check_call(["cc", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include"),
                           "-L", os.path.join(ROOT, "bystro-vcf_amd"), "-lbvcf",
                           "-Wl,-rpath," + os.path.join(ROOT, "bystro-vcf_amd")])
    out = subprocess.check_output([str(exe)]).decode().split()
    no_out, out_bgzf, reserved3, size = map(int, out[:4])
    assert out_bgzf == bv.Config.out_bgzf.offset == no_out + 1
    assert reserved3 == bv.Config.reserved3.offset and bv.Config.reserved3.size == 2
    assert size == C.sizeof(bv.Config)
    assert int(out[4]) == 0  # the default leaves the output plain
    c = bv.make_config({"compressOutput": "bgzf"})
    assert c.out_bgzf == 1 and bv.make_config().out_bgzf == 0
