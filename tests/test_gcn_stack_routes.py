"""The routing of ``mgcn.ops._GCNStack``, pinned case by case
(tests/gcn_stack_cases.py) against tests/golden/gcn_stack_launches.json: on the
host the planner's routes and their invariants, on the device the libmgcn
launches one forward + backward makes.  A change that moves a route on
purpose re-records the file and shows the difference in review."""
import pytest
import torch

import gcn_stack_cases as C

GOLD = C.load_golden()
IDS = [c.name for c in C.CASES]


def test_golden_file_covers_the_case_table():
    assert sorted(GOLD["cases"]) == sorted(IDS)
    assert sorted(GOLD["graphs"]) == sorted(C.GRAPHS)
    # the two hub graphs put their heavy row in one view each
    assert [bool(GOLD["graphs"][k][v]) for k in C.GRAPHS for v in ("n_heavy_fwd", "n_heavy_bwd")] \
        == [False, False, False, True, True, False]


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_plan_stack_routes(case):
    """No device: the planner sees shapes, flags and three numbers per view."""
    import mgcn
    from mgcn import ops
    from mgcn.ops import _Bwd, _TopBias
    mgcn.load()  # the host-side *_supported probes
    views = C.stub_views(**GOLD["graphs"][case.graph])
    plan = C.plan_case(case, ops, *views)
    assert C.routes(plan) == GOLD["cases"][case.name]["routes"]
    layers, top = plan.layers, len(plan.layers) - 1
    for l, lp in enumerate(layers):
        # Z is kept iff the backward forms dW from it
        assert lp.keep_z == (lp.bwd is _Bwd.Z_FORM), l
        # a mask is written iff the layer above reads it in its dX epilogue (the
        # wide dX-only adjoint's 8-word mask included), and that layer forms a dX
        assert lp.write_mask == (l < top and layers[l + 1].epilogue), l
        assert not lp.write_mask or case.acts[l] == "relu"
        if lp.epilogue:
            assert lp.bwd not in (_Bwd.NONE, _Bwd.FULL_DW, _Bwd.GEMM_BWD_DW), l
            assert lp.bwd is not _Bwd.DX_ONLY or not lp.want_dw
        assert lp.want_dw == (l not in case.frozen) and lp.want_dx == (l > 0 or case.x_grad)
        assert lp.winner_bits == (case.aggr == "max")  # max never takes the fused forward
    # the top bias gradient has exactly one source, and that launch exists
    assert isinstance(plan.top_bias, _TopBias)
    if plan.top_bias is not _TopBias.COLSUM_PASS:
        assert case.acts[top] == "none" and case.aggr != "mean"
    assert (plan.top_bias is _TopBias.TOP_DW_PASS) == \
        (layers[top].bwd is _Bwd.Z_FORM and case.acts[top] == "none" and case.aggr != "mean")
    if plan.top_bias is _TopBias.ADJOINT:
        assert layers[top].bwd is _Bwd.FULL and case.bias
    if plan.top_bias is _TopBias.BOTTOM_DW_PASS:
        assert top > 0 and layers[0].bwd is _Bwd.Z_FORM and case.bias
    if case.default_switches and case.all_grads:
        # pure: a second call, after other cases ran, plans every layer alike
        assert C.plan_case(case, ops, *views) == plan


@pytest.fixture(scope="module")
def plans(cuda):
    from mgcn.graph import plan_for
    out = {}
    for kind in C.GRAPHS:
        plan = plan_for(torch.from_numpy(C.edge_index(kind)).to(cuda), C.N)
        out[kind] = (plan, plan.norm("sm"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_gcn_stack_launches(cuda, plans, case):
    from mgcn import ops
    plan, norm = plans[case.graph]
    assert {"n_heavy_fwd": plan.fwd.n_heavy, "n_heavy_bwd": plan.bwd.n_heavy} == \
        GOLD["graphs"][case.graph]
    launches, out = C.run_case(case, ops, plan, norm, cuda)
    assert launches == GOLD["cases"][case.name]["launches"]
    assert all(bool(torch.isfinite(t).all()) for t in out.values())
