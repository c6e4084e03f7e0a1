"""The launch geometry of the wave-tile sweeps (dl_esm_inf_amd/csrc/dlesm_tile_plan.h) against the expressions the launchers
held before it, under AddressSanitizer + UBSan on the CPU (harness tests/tile_plan_host.cpp, a stand-alone program)."""
import os
import re
import subprocess

from conftest import ROOT


def test_tile_plan_matches_the_launchers_it_replaced(tmp_path):
    exe = tmp_path / "tile_plan_host"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dl_esm_inf_amd", "csrc"),
           os.path.join(ROOT, "tests", "tile_plan_host.cpp"), "-o", str(exe)]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    m = re.search(r"checks passed: (\d+) comparisons", p.stdout)
    assert m and int(m.group(1)) > 100_000_000, p.stdout[-2000:]
