"""GPU test (-m gpu): the Fortran wrappers of the NEMOLite2D-class time step that skips land through a
small program (tests/fortran/ftest_nemolite_wet.f90, built by the Fortran layer's Makefile like every program there).  On a
masked channel with an island and a land block 420 columns wide, with DL_ESM_ALIGNMENT=64 (the sweep), five steps of
invoke_nemolite_step / invoke_nemolite_step_dm with skip_land = .true. against the same steps without it: ssha_u, ssha_v, ua
and va hold the same bits in every cell, ssha wherever tmask /= 0 (an argument out of order in the bind(C) interfaces or
the wrappers shows up as a differing array); the plan has inactive tiles, and land ssha was left alone."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_nemolite_wet.exe")


def test_fortran_skip_land_obeys_the_contract():
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    env["DL_ESM_ALIGNMENT"] = "64"
    p = subprocess.run([EXE, "560", "48"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "G: steps compared, 0 arrays differ" in p.stdout, p.stdout[-3000:]
    assert "differs" not in p.stdout and "never written" not in p.stdout, p.stdout[-3000:]
    m = re.search(r"G: wet plan: (\d+) tiles, (\d+) active", p.stdout)
    assert m and 0 < int(m.group(2)) < int(m.group(1)), p.stdout[-3000:]
    m = re.search(r"G: land ssha kept in (\d+) cells", p.stdout)
    assert m and int(m.group(1)) > 0, p.stdout[-3000:]
