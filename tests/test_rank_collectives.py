"""CPU test: the cross-rank tail of the diagnostics in dl_esm_inf_amd/parallel_mod.py (global_sum, global_max, _global_count,
_owner, _place, _where) as rank r of N for N = 1, 2, 4 and every r, without a GPU and without other processes.  _cabi.lib is
replaced by a fake whose two collectives combine the caller's value with a scripted list of what the other ranks pass, in call
order; the script comes from the rule as DESIGN.md section 6.14 states it (written out in `_others`, independently of the code
under test), the expected results from closed forms.  At N = 1 the fake must never be called."""
import pytest

import dl_esm_inf_amd  # noqa: F401
from dl_esm_inf_amd import _cabi, parallel_mod

NX = 13                                     # row length of the local arrays: index = (j - 1) * NX + (i - 1)
WORLDS = [(n, r) for n in (1, 2, 4) for r in range(1, n + 1)]


class FakeLib:
    """dlesm_global_sum_f64 / dlesm_global_max_f64 over the caller's value and script[call number]"""

    def __init__(self, script):
        self.script, self.calls = list(script), []

    def _entry(self, name, combine):
        def call(ref):
            others = self.script[len(self.calls)]
            assert others[0] == name, (len(self.calls), name, others[0])
            self.calls.append(name)
            ref._obj.value = combine([ref._obj.value] + list(others[1]))
            return 0
        return call

    def __getattr__(self, name):
        if name == "dlesm_global_sum_f64":
            return self._entry("sum", sum)
        if name == "dlesm_global_max_f64":
            return self._entry("max", max)
        raise AttributeError(name)


@pytest.fixture
def world(monkeypatch):
    def enter(n, r, script=()):
        fake = FakeLib(script)
        monkeypatch.setattr(parallel_mod, "_rank", r)
        monkeypatch.setattr(parallel_mod, "_nranks", n)
        monkeypatch.setattr(_cabi, "lib", lambda: fake)
        return fake
    return enter


def _others(tops, indexes, r):
    """what the ranks other than r pass to the four collectives of _place, by the rule: a rank holds the extreme when it has
    a cell and its top is the global one; the owner is the lowest such rank; only the owner passes its i and j"""
    n, top = len(tops), max(tops)
    holds = [indexes[q] >= 0 and tops[q] == top for q in range(n)]
    owner = min([q + 1 for q in range(n) if holds[q]], default=None)
    rest = [q for q in range(n) if q + 1 != r]
    return [("max", [tops[q] for q in rest]),
            ("max", [-float(q + 1) if holds[q] else -1.0e9 for q in rest]),
            ("sum", [float(indexes[q] % NX + 1) if q + 1 == owner else 0.0 for q in rest]),
            ("sum", [float(indexes[q] // NX + 1) if q + 1 == owner else 0.0 for q in rest])]


def _index(q):
    return 100 + q                          # rank q's cell: a different i and j on every rank


def _ij(q):
    return (_index(q) % NX + 1, _index(q) // NX + 1)


# name -> (tops(n), indexes(n), expected (top, at)(n)); ranks q = 1 .. n
CASES = {
    "all tie, all hold": (lambda n: [2.5] * n, lambda n: [_index(q) for q in range(1, n + 1)],
                          lambda n: (2.5, (1,) + _ij(1))),
    "distinct tops": (lambda n: [0.25 * q for q in range(1, n + 1)], lambda n: [_index(q) for q in range(1, n + 1)],
                      lambda n: (0.25 * n, (n,) + _ij(n))),
    "tie, rank 1 holds none": (lambda n: [2.5] * n, lambda n: [-1] + [_index(q) for q in range(2, n + 1)],
                               lambda n: (2.5, (2,) + _ij(2) if n > 1 else None)),
    "nobody holds one": (lambda n: [0.0] * n, lambda n: [-1] * n, lambda n: (0.0, None)),
    # a minimum as the maximum of its negative: depths 10 + q, the shallowest on rank 1
    "negated": (lambda n: [-(10.0 + q) for q in range(1, n + 1)], lambda n: [_index(q) for q in range(1, n + 1)],
                lambda n: (-11.0, (1,) + _ij(1))),
    # rank 1 has a cell but a top below the global one (the last rank's): it does not own
    "lower top does not own": (lambda n: [1.0] + [3.0] * (n - 1), lambda n: [_index(q) for q in range(1, n + 1)],
                               lambda n: (3.0, (2,) + _ij(2)) if n > 1 else (1.0, (1,) + _ij(1))),
}


@pytest.mark.parametrize("n,r", WORLDS)
@pytest.mark.parametrize("case", list(CASES))
def test_place(world, case, n, r):
    tops, indexes, want = (f(n) for f in CASES[case])
    fake = world(n, r, _others(tops, indexes, r))
    got = parallel_mod._place(tops[r - 1], indexes[r - 1], NX)
    assert got == want, (case, n, r)
    assert fake.calls == (["max", "max", "sum", "sum"] if n > 1 else [])


@pytest.mark.parametrize("n,r", WORLDS)
def test_owner_alone(world, n, r):
    """the half run_health uses: ranks 2 and up pass here = True with (i, j) = (10 + q, 20 + q)"""
    here = [q >= 2 for q in range(1, n + 1)]
    rest = [q for q in range(1, n + 1) if q != r]
    fake = world(n, r, [("max", [-float(q) if here[q - 1] else -1.0e9 for q in rest]),
                        ("sum", [12.0 if q == 2 else 0.0 for q in rest]), ("sum", [22.0 if q == 2 else 0.0 for q in rest])])
    got = parallel_mod._owner(here[r - 1], 10 + r, 20 + r)
    assert got == ((2, 12, 22) if n > 1 else None)
    assert fake.calls == (["max", "sum", "sum"] if n > 1 else [])


@pytest.mark.parametrize("n,r", WORLDS)
def test_counts_sum_exactly(world, n, r):
    rest = [q for q in range(1, n + 1) if q != r]
    fake = world(n, r, [("sum", [float(2**40 + q) for q in rest])])
    got = parallel_mod._global_count(2**40 + r)
    assert isinstance(got, int) and got == n * 2**40 + n * (n + 1) // 2
    assert fake.calls == (["sum"] if n > 1 else [])


@pytest.mark.parametrize("n,r", WORLDS)
def test_global_sum_and_max(world, n, r):
    rest = [q for q in range(1, n + 1) if q != r]
    fake = world(n, r, [("sum", [0.5 * q for q in rest]), ("max", [-1.5 * q for q in rest])])
    assert parallel_mod.global_sum(0.5 * r) == 0.25 * n * (n + 1)
    assert parallel_mod.global_max(-1.5 * r) == -1.5
    assert fake.calls == (["sum", "max"] if n > 1 else [])


def test_a_failing_collective_raises(world, monkeypatch):
    """the C entry's status goes through _cabi.check"""
    class Failing:
        def dlesm_global_max_f64(self, ref):
            return _cabi.EINVAL

        def dlesm_last_error(self):
            return b"no communicator"
    world(2, 1)
    monkeypatch.setattr(_cabi, "lib", Failing)
    with pytest.raises(_cabi.DlesmError, match="no communicator"):
        parallel_mod.global_max(1.0)


def test_where():
    assert parallel_mod._where((3, 7, 9)) == "at local (i, j) = (7, 9) on rank 3"
    assert parallel_mod._where(None) == "nowhere"
