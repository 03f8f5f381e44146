"""``_backward_plan`` -- the backward's route decision, from numbers alone -- on the cases of
tests/test_backward_routes_gpu.py, without a device, against the same tests/golden/backward_routes.json (recorded from the
shim as it was before the decision became a function; not edited).  The library's host-only queries need no GPU
(tests/test_capi.py relies on that too).

From the recorded calls of a case: the route (which entry points were called), the flags (of the calls that carry
them; the staged entry points carry none, so a staged case answers for the flags of its one-call twin), the stage bits
or entry points in order, and the names in the event log.  Two more cases that no few-second GPU test can run -- a value
slab over 2 GiB -- are written from the recorded shim's source, as said there."""
import pytest
import torch

import MultiScaleDeformableAttention as MSDA
from test_backward_routes_gpu import CASES, DTYPES, KNOBS, RUNS, golden, level_tables, run_id

ROUTE_OF = {"mmfs_msda_backward_sorted": "sorted", "mmfs_msda_backward_hybrid": "hybrid",
            "mmfs_msda_backward_taps": "staged", "mmfs_msda_backward_checked": "library"}
FALL_BACK = "mmfs_msda_backward_checked"


def set_knobs(monkeypatch, knobs, with_log):
    for knob, v in {**KNOBS, **knobs}.items():
        monkeypatch.setattr(MSDA, knob, v)
    monkeypatch.setattr(MSDA, "_ws_cache", {})
    monkeypatch.setattr(MSDA, "_event_log", [] if with_log else None)


def numbers(c):
    """A case as ``_backward_plan`` sees it: (code, dims, slab_bytes, info, lazy_zero_attn).  ``info`` comes from the
    shim's own registry, on host tensors: what the GPU test's registration leaves behind."""
    sh, st, S = level_tables(c)
    dt = DTYPES[c["dtype"]]
    info = None
    if c["table"] != "fresh":
        MSDA.register_level_tables(sh, st, S, host_shapes=sh.clone(), host_start=st.clone())
        info = MSDA._level_info(sh, st, S, sync=False)
        assert info is not None and info[0] == (c["table"] == "registered")
    dims = (c["B"], S, c["H"], c["D"], sh.shape[0], c["Nq"], c["P"])
    return MSDA._DTYPE_CODE[dt], dims, S * c["H"] * c["D"] * torch.empty((), dtype=dt).element_size(), info, c["lazy"]


@pytest.mark.parametrize("name,with_log", RUNS, ids=[run_id(*r) for r in RUNS])
def test_plan_is_the_recorded_route(name, with_log, monkeypatch):
    c, want = CASES[name], golden()[run_id(name, with_log)]
    set_knobs(monkeypatch, c["knobs"], with_log)
    if not want["calls"]:                       # raised before any call: the plan raises the same thing
        with pytest.raises(RuntimeError) as e:
            MSDA._backward_plan(*numbers(c))
        assert str(e.value) == want["raises"]
        return
    plan = MSDA._backward_plan(*numbers(c))
    calls = want["calls"]
    assert plan.route == ROUTE_OF[calls[0]["entry"]]
    assert (plan.route == "sorted") == (want["sorted"] == 1)
    # the route's own calls: all of them, unless one was refused and the recorded shim fell back to the library call
    own = calls if plan.route == "library" else [k for k in calls if k["entry"] != FALL_BACK]
    fell_back = len(own) < len(calls)
    assert len(calls) - len(own) <= 1 and (not fell_back or calls[-1]["entry"] == FALL_BACK)
    stages = [k["stages"] if "stages" in k else k["entry"] for k in own]
    planned = [stage for _, stage in plan.stages]
    assert stages == (planned[:len(stages)] if fell_back else planned)
    if with_log:
        names = want["log"][:len(own)]
        assert names == [n for n, _ in plan.stages][:len(names)]
        if fell_back:
            assert want["log"][len(own):] == ["msda_bwd_atomic"]
    # flags: of every recorded call that has them (the fall-back's included); a staged case's from its one-call twin
    flagged = calls if plan.route != "staged" else golden()[run_id(name, False)]["calls"]
    assert {k["flags"] for k in flagged if "flags" in k} == {plan.flags}
    assert (plan.ws_bytes == 0) == own[-1].get("ws_null", plan.ws_bytes == 0)
    assert plan.status_word == (not calls[-1].get("word_null", True))


BIG = dict(code=2, dims=(1, 1 << 21, 8, 128, 1, 64, 4))         # bf16, S*H*D*2 = 4 GiB in one batch row


def big_plan(monkeypatch, taps_algo):
    set_knobs(monkeypatch, {"_taps_algo": taps_algo}, False)
    sh, st = torch.tensor([[1024, 2048]]), torch.tensor([0])
    B, S, H, D, L, Nq, P = BIG["dims"]
    info = MSDA.register_level_tables(sh, st, S, host_shapes=sh.clone(), host_start=st.clone())
    assert info[0]
    slab = S * H * D * 2
    assert slab > 0x7fffffff
    return MSDA._backward_plan(BIG["code"], BIG["dims"], slab, info, False)


def test_lds_named_for_a_slab_over_the_limit_becomes_the_row_gather(monkeypatch):
    """The recorded shim, lines 665-668: ``taps == "lds"`` and a slab over _MAX_SLAB_BYTES -> ``taps = "gather"``: the
    flags carry _BWD_TAPS_ROW_GATHER, not _BWD_TAPS_LDS_LEVELS, and nothing raises."""
    plan = big_plan(monkeypatch, "lds")
    assert plan.flags & MSDA._TAPS_FLAGS["gather"] and not plan.flags & MSDA._TAPS_FLAGS["lds"]
    assert plan.flags & MSDA._BWD_CANONICAL_LEVELS


def test_sorted_named_for_a_slab_over_the_limit_goes_on_to_the_other_routes(monkeypatch):
    """The recorded shim, lines 700-705: the "does not apply" error exempts a slab over _MAX_SLAB_BYTES; the call goes
    on to the routes below.  (The sorted query refuses such a slab; so does the hybrid one.)"""
    plan = big_plan(monkeypatch, "sorted")
    assert plan.route in ("hybrid", "library") and len(plan.stages) == 1
    assert plan.flags & MSDA._BWD_CANONICAL_LEVELS and not plan.flags & (MSDA._TAPS_FLAGS["gather"] | MSDA._TAPS_FLAGS["lds"])
    # under the limit the same arguments but fp32 storage raise
    set_knobs(monkeypatch, {"_taps_algo": "sorted"}, False)
    with pytest.raises(RuntimeError, match="does not apply"):
        MSDA._backward_plan(0, BIG["dims"], 0x7fffffff, None, False)
