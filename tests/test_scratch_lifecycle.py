"""The context's scratch-buffer types (nghttp3_amd/csrc/qh_scratch.h: reserve /
release, the code qh_api.inc runs over hipMalloc; the layout and staging
types every batch entry point cuts its buffers with) driven over malloc by a
stand-alone program built with AddressSanitizer and UBSan
(tests/c/scratch_lifecycle.cc).  CPU only."""
import os
import subprocess

from conftest import ROOT


def test_scratch_lifecycle_under_sanitizers(tmp_path):
    exe = tmp_path / "scratch_lifecycle"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nghttp3_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "scratch_lifecycle.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "scratch lifecycle ok: 4 policies, 8 layouts, staging" in out.stdout
