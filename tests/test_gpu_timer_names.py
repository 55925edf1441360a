"""The kernel-timer contract of mgcn.ops, over every timed launch family
(tests/timer_names_cases.py): each start call has its stop, and the names and
the (rows, edges) the starts carry -- what bench.py's per-kernel table and
byte accounting read -- are those recorded before mgcn/ops.py was split
(tests/golden/ops_timer_names.json)."""
import pytest

import timer_names_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(cuda):
    from mgcn import ops
    return tc.run_all(ops, cuda)


@pytest.mark.parametrize("case", list(tc.CASES))
def test_every_start_has_its_stop(recorded, case):
    events, _ = recorded[case]
    assert len(events) % 2 == 0  # (bmm and segment_mean launch untimed kernels only: none)
    for start, stop in zip(events[0::2], events[1::2]):
        assert start[1] is True and stop == [start[0], False, None, None], (start, stop)


def test_names_rows_and_edges_match_the_recording(recorded):
    golden = tc.load_golden()
    assert list(golden) == list(tc.CASES)
    for case, (events, _) in recorded.items():
        assert tc.launches(events) == golden[case], case
