"""The 22 view-walking attention entries (soft and hard x fwd, edge_softmax,
bwd_dst, bwd_src x plain, _bf16, _sched) answer bad arguments and no-ops as
recorded in tests/golden/attention_entry_errors.json: the same return code and
the same mgcn_last_error() text, so the order of the host checks, every
message and its entry-name prefix are pinned.  The table of calls is
scripts/record_attention_entry_errors.py's; the golden file was recorded with
that script on the commit before the entries came to share one checked body
per operation.

Every pointer is a dummy.  A recorded case returns before any launch; if an
entry lost a check, the call would become a launch on that pointer.  That must
never happen where a device exists, so the test runs only where none does."""
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(torch.cuda.is_available(),
                                reason="dummy pointers: replayed only where no device exists")


def _recorder():
    path = os.path.join(ROOT, "scripts", "record_attention_entry_errors.py")
    spec = importlib.util.spec_from_file_location("record_attention_entry_errors", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
CASES = REC.cases()
with open(os.path.join(ROOT, "tests", "golden", "attention_entry_errors.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    import mgcn
    return mgcn.load()


def test_the_table_is_the_recorded_one():
    assert len(CASES) == 22
    assert {e: sorted(t) for e, t in CASES.items()} == {e: sorted(t) for e, t in GOLDEN.items()}
    from mgcn import _lib as L
    for entry, table in GOLDEN.items():
        for case, (rc, err) in table.items():
            # what the recorder accepts: a refusal, or a listed no-op
            assert rc == L.EINVAL or (rc == L.OK and CASES[entry][case][1] and err == ""), \
                (entry, case)


@pytest.mark.parametrize("entry", sorted(CASES))
def test_entry_answers_as_recorded(lib, entry):
    for case, (args, _noop) in CASES[entry].items():
        assert REC.call(lib, entry, args) == GOLDEN[entry][case], (entry, case)
