"""The window arithmetic of the hand-over tests (tests/handover_load.py: overlap_counts, window_is_loaded) on made-up logs:
a pass window counts as tested under load only with a completed load launch before it, at least three inside and one after."""
from handover_load import MIN_INSIDE, overlap_counts, window_is_loaded


def test_counts_inside_outside_and_on_the_ends():
    log = [10, 20, 30, 40, 50, 60, 70]
    assert overlap_counts(log, 25, 55) == (2, 3, 2)
    assert overlap_counts(log, 20, 60) == (1, 5, 1)          # the ends belong to the window
    assert overlap_counts(log, 0, 100) == (0, 7, 0)
    assert overlap_counts(log, 71, 80) == (7, 0, 0)
    assert overlap_counts(log, 1, 9) == (0, 0, 7)
    assert overlap_counts([], 1, 9) == (0, 0, 0)


def test_a_window_inside_the_load_is_loaded():
    assert MIN_INSIDE == 3
    log = list(range(0, 1000, 10))
    assert window_is_loaded(log, 105, 135)                   # 110, 120, 130 inside
    assert not window_is_loaded(log, 105, 129)               # two inside
    assert window_is_loaded(log, 105, 129, min_inside=2)


def test_a_window_outside_the_load_is_void():
    log = [100, 110, 120, 130, 140]
    assert not window_is_loaded(log, 10, 50)                 # the load started after the window
    assert not window_is_loaded(log, 200, 300)               # ... or had stopped before it
    assert not window_is_loaded(log, 141, 150)


def test_a_window_that_straddles_an_end_of_the_load_is_void():
    log = [100, 110, 120, 130, 140]
    assert not window_is_loaded(log, 50, 135)                # four inside, one after, none before: began without the load
    assert not window_is_loaded(log, 105, 500)               # four inside, one before, none after: outlived the load
    assert not window_is_loaded(log, 50, 500)                # the load lies wholly inside
    assert window_is_loaded(log, 101, 139)


def test_empty_logs_and_empty_windows_are_void():
    assert not window_is_loaded([], 0, 100)
    assert not window_is_loaded([5, 6, 7, 8, 9], 7, 7)       # an empty window
    assert not window_is_loaded([5, 6, 7, 8, 9], 8, 6)       # a reversed one
