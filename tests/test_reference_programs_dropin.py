"""Drop-in check of the Fortran API layer: the reference's OWN programs -- its example and its four test programs --
compiled UNMODIFIED against this library's modules (dl_esm_inf_amd/fortran/build/*.mod + lib_fd_hip.a +
libdlesm_hip.so) by build() (oracle/Makefile target `dropin`, into oracle/_ref/dropin; nothing of them is copied into the
repository) and run on one rank.  What this pins is the API surface a GOcean application sees: module names, type
components, generic interfaces, argument lists, the device-sync callback seam (tests/device_computation/test_device_io.f90
installs its own callbacks) and the one-rank behaviour of decomposition, halo exchange, global sum, scatter and gather.

CPU only (-m "not gpu"): on one rank these programs keep their fields on the host -- no kernel of the hot path is
invoked, so no GPU is needed; tests/test_a_reference_programs_multirank_gpu.py runs the same executables on 2-6 ranks.
Skipped where build() found no reference sources to compile them from."""
import os
import subprocess

import pytest

from conftest import ROOT, load_golden

DROP = os.path.join(ROOT, "oracle", "_ref", "dropin")

PROGRAMS = ("model", "test_device_io", "test_halos", "test_gsum", "test_reduction")


@pytest.fixture(scope="module")
def built():
    exes = {name: os.path.join(DROP, f"{name}.exe") for name in PROGRAMS}
    missing = [e for e in exes.values() if not os.path.exists(e)]
    if missing:
        pytest.skip(f"{missing[0]} not built (build() makes it where the reference's sources are present)")
    return exes


def _run(exe, **env):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DL_ESM_ALIGNMENT"):
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    p = subprocess.run([exe], env=e, capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout + p.stderr


def test_reference_example_model(built):
    """example/model.f90: 4 x 10 domain, the four point types filled with 1.0 -- every checksum is 40 (model.f90:95-98)"""
    rc, out = _run(built["model"])
    assert rc == 0, out[-2000:]
    sums = [ln for ln in out.splitlines() if "checksum" in ln]
    assert len(sums) == 4 and all("0.40000000E+02" in ln for ln in sums), out[-2000:]
    assert "Example model set-up complete" in out


@pytest.mark.parametrize("alignment", [None, 1, 2, 4, 8, 12, 16, 64])
def test_reference_device_io_test(built, alignment):
    """tests/device_computation/test_device_io.f90: its own 'virtual device' behind the read/write callbacks of the
    field type.  The program says it must pass for any DL_ESM_ALIGNMENT; with the REAL reference library (the same
    source, outcomes recorded in tests/golden/ref_device_io.json by oracle/make_golden.py) it passes up to 12 and overruns
    its fixed-size virtual device from 16 on ('free(): corrupted ...').  Required here: pass up to 12, and the same
    outcome as the real reference beyond."""
    env = {} if alignment is None else {"DL_ESM_ALIGNMENT": alignment}
    rc, out = _run(built["test_device_io"], **env)
    ok = rc == 0 and "Test passed" in out
    if alignment is None or alignment <= 12:
        assert ok, out[-2000:]
        return
    real = next(o for o in load_golden("ref_device_io")["outcomes"] if o["alignment"] == alignment)
    assert ok == real["passed"], (out[-800:], real)


@pytest.mark.parametrize("nx,ny", [(10, 4), (4, 10), (10, 10)])
def test_reference_dist_mem_programs_on_one_rank(built, nx, ny):
    """tests/dist_mem/{test_halos, test_gsum, test_reduction}.f90 with the domain sizes of the reference's Makefile
    (10x4, 4x10, 10x10), one rank: no ERROR line, sums equal the number of cells, scatter and gather come back right"""
    for name in ("test_halos", "test_gsum", "test_reduction"):
        rc, out = _run(built[name], JPIGLO=nx, JPJGLO=ny)
        assert rc == 0, (name, out[-2000:])
        assert "ERROR" not in out, (name, out[-2000:])
        if name == "test_gsum":
            lines = [ln for ln in out.splitlines() if "Global sum" in ln]
            vals = [float(ln.split(":")[-1]) for ln in lines]
            assert len(vals) == 4 and all(v == float(nx * ny) for v in vals), (vals, out[-1500:])
        if name == "test_reduction":
            assert "Field distributed correctly" in out and "Field gathered correctly" in out, out[-1500:]
