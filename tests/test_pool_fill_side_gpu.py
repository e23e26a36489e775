"""Every device call of tests/side_runs.py (the functions of the side headers, include/tgx_*.h) on hostile memory: the loop
of tests/test_pool_fill_gpu.py over the second registry.  Under TGX_POOL_FILL every buffer the library's pool hands out
holds 0, 255 or 1 before its owner sees it; each run passes the entry's check, tgx_pool_filled_bytes() grew in each, and
the outputs under 255 and 1 are bit for bit the control's.  These calls take their scan records, walk buffers, head flags,
sort room and histograms from the pool without clearing them: a tail that nothing wrote, a pre-set that covers less than
its array or a histogram that relies on zeros shows here and nowhere else."""
import pytest

pytestmark = pytest.mark.gpu

import tokengeex_amd as tgx
from tokengeex_amd import _lib

import side_runs
from test_pool_fill_gpu import FILLS, KNOB, same_outputs


@pytest.mark.parametrize("name", sorted(side_runs.ENTRIES))
def test_entry_on_filled_memory(monkeypatch, name):
    e = side_runs.ENTRIES[name]
    assert not e.env and e.deterministic
    ctx = side_runs.Ctx()
    tgx.pool_trim()
    runs = {}
    for fill in FILLS:
        monkeypatch.setenv(KNOB, fill)
        before = _lib.pool_filled_bytes()
        out = e.run(ctx)
        assert _lib.pool_filled_bytes() > before, (name, fill, "nothing was filled")
        e.check(out)
        runs[fill] = out
    for fill in FILLS[1:]:
        same_outputs(e, runs[fill], runs["0"], fill)
