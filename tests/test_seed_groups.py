"""CPU: how ace_zero.py --seed_parallel_workers splits the seed trials into training groups (session.seed_groups)."""
import pytest

from acezero_amd.session import seed_groups


@pytest.mark.parametrize("workers, groups", [
    (1, [[0], [1], [2], [3], [4]]),
    (3, [[0, 1, 2], [3, 4]]),
    (-1, [[0, 1, 2, 3, 4]]),
    (8, [[0, 1, 2, 3, 4]]),
    (20, [[0, 1, 2, 3, 4]]),
])
def test_five_seeds(workers, groups):
    assert seed_groups(5, workers) == groups


def test_groups_are_capped_at_eight_members():
    assert seed_groups(10, -1) == [list(range(8)), [8, 9]]
    assert seed_groups(10, 20) == [list(range(8)), [8, 9]]
    assert seed_groups(0, 3) == []


@pytest.mark.parametrize("workers", [0, -2, -5])
def test_bad_worker_counts_are_refused(workers):
    with pytest.raises(ValueError):
        seed_groups(5, workers)


def test_reconstruct_refuses_a_bad_worker_count_before_any_work():
    from acezero_amd import session

    class _NoWork(session.ReconstructionSession):
        def __init__(self):
            self.opt = session.default_options()

        def map(self, *a, **k):
            raise AssertionError("mapped before the argument was checked")

    with pytest.raises(ValueError):
        _NoWork().reconstruct(seed_parallel_workers=0)
