"""The heavy-row route of the fp32 attention launches on the MI355X
(mgcn_(h)att_*_sched, csrc/attention_heavy.hip): every tensor soft and hard
(training) attention produce has, with the route on, the bits the wave-per-row
kernels give it (``torch.equal``: no tolerance), on a graph with one row of
every degree around the heavy (128) and the giant (512) thresholds in both
views; plus the fp64 restatement's bound (a route wrong in the same way on and
off), repeatability, the C ABI with leading dimensions and guard bands, the
routing (which C entry runs when), and the models."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from attention_ref import att_ref, check
from hard_attention_ref import hatt_ref

pytestmark = pytest.mark.gpu

DEGREES = (127, 128, 129, 191, 192, 193, 511, 512, 513, 1000, 2100)
POOL = 128
ND = len(DEGREES)
SCHED = ("mgcn_att_fwd_sched", "mgcn_edge_softmax_sched", "mgcn_att_bwd_dst_sched",
         "mgcn_att_bwd_src_sched", "mgcn_hatt_fwd_sched", "mgcn_hatt_edge_softmax_sched",
         "mgcn_hatt_bwd_dst_sched", "mgcn_hatt_bwd_src_sched")
_HUB = {}


def hub_ladder(cuda):
    """(edge_index on the GPU, N, plan): 128 pool nodes with 400 random edges
    among themselves, one node of every in-degree and one of every out-degree
    in DEGREES (the other endpoints drawn with replacement from the pool:
    parallel edges occur), 3 isolated nodes, shuffled COO order (the recipe of
    test_gpu_edge_gate_heavy.py)."""
    if "g" not in _HUB:
        from mgcn.graph import plan_for
        rng = np.random.default_rng(71)
        N = POOL + 2 * ND + 3
        parts = [rng.integers(0, POOL, (2, 400))]
        for i, d in enumerate(DEGREES):
            parts.append(np.stack([rng.integers(0, POOL, d), np.full(d, POOL + i)]))
            parts.append(np.stack([np.full(d, POOL + ND + i), rng.integers(0, POOL, d)]))
        ei = np.concatenate(parts, axis=1)
        ei = ei[:, rng.permutation(ei.shape[1])]
        ind, outd = np.bincount(ei[1], minlength=N), np.bincount(ei[0], minlength=N)
        assert tuple(ind[POOL:POOL + ND]) == DEGREES and not outd[POOL:POOL + ND].any()
        assert tuple(outd[POOL + ND:POOL + 2 * ND]) == DEGREES and not ind[POOL + ND:N].any()
        assert ind[:POOL].max() < 128 and outd[:POOL].max() < 128
        assert not ind[N - 3:].any() and not outd[N - 3:].any()
        pairs = ei[0] * N + ei[1]
        assert len(np.unique(pairs)) < pairs.size  # parallel edges
        eig = torch.from_numpy(ei.astype(np.int64)).to(cuda)
        plan = plan_for(eig, N)
        for view in (plan.fwd, plan.bwd):  # 129 .. 2100 heavy, 513 / 1000 / 2100 giant
            assert view.order is not None and (view.n_heavy, view.n_giant) == (9, 3)
        _HUB["g"] = (eig, N, plan)
    return _HUB["g"]


@contextlib.contextmanager
def route(on, calls=None):
    """The heavy-row switch set to ``on``; with ``calls`` (a dict), every
    mgcn_*_sched attribute of the library object wrapped to count its calls
    (ops_attention looks the entries up per call)."""
    import mgcn
    from mgcn import ops
    lib = mgcn.load()
    before = ops.attention_heavy_rows()
    ops.set_attention_heavy_rows(on)
    saved = {}
    if calls is not None:
        for name in SCHED:
            fn = getattr(lib, name)
            saved[name] = fn

            def counted(*a, _fn=fn, _name=name):
                calls[_name] = calls.get(_name, 0) + 1
                return _fn(*a)
            setattr(lib, name, counted)
    try:
        yield
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)
        ops.set_attention_heavy_rows(before)


def masked_group(adir):
    """The node whose softmax group (degree 513: heavy and giant) the mask
    zeroes, and the COO row of ei that names a group's node."""
    return (POOL + 8, 1) if adir == "in" else (POOL + ND + 8, 0)


def inputs(cuda, H, C, adir, mask, seed):
    ei, N, plan = hub_ladder(cuda)
    E = plan.nnz
    gen = torch.Generator().manual_seed(2000 + seed)
    Hp = torch.randn(N, H * C, generator=gen)
    att = torch.randn(1, H, 2 * C, generator=gen) * 0.5
    dY = torch.randn(N, H * C, generator=gen)
    noise = -torch.log(-torch.log(torch.rand(E, H, generator=gen).clamp(1e-6, 1 - 1e-6)))
    m = None
    if mask:  # dropout at p = 0.5 with its scale, one whole heavy group dropped
        m = (torch.rand(E, H, generator=gen) < 0.5).float() * 2.0
        node, side = masked_group(adir)
        m[ei[side].cpu() == node] = 0.0
    return Hp, att, dY, noise, m


def run_op(cuda, kind, H, C, adir, act, mask, seed=0, dtype=torch.float32):
    """attention_aggregate / hard_attention_aggregate(training, T = 0.5)
    forward + backward on the hub ladder: Y, alpha_coo, dHp, datt."""
    from mgcn.ops import attention_aggregate, hard_attention_aggregate
    _, _, plan = hub_ladder(cuda)
    Hp, att, dY, noise, m = inputs(cuda, H, C, adir, mask, seed)
    Hp = Hp.to(cuda).to(dtype).requires_grad_(True)
    att = att.to(cuda).requires_grad_(True)
    m = None if m is None else m.to(cuda)
    if kind == "soft":
        Y, alpha = attention_aggregate(Hp, att, plan, H, act, adir, edge_mask=m)
    else:
        Y, alpha = hard_attention_aggregate(Hp, att, plan, H, act, adir, 0.5, training=True,
                                            noise=noise.to(cuda), edge_mask=m)
    Y.backward(dY.to(cuda).to(dtype))
    torch.cuda.synchronize()
    return {"Y": Y.detach(), "alpha_coo": alpha, "dHp": Hp.grad, "datt": att.grad}


# (H, C, att_dir, act, edge mask).  The kernels branch on (H, C) -- H = 1 and
# odd C; H not a power of two (G = 21, a dead lane, head_sum's lane-group
# branch); the botnet shape; the segmented butterfly at 2 features per lane;
# C a power of two > 64 (generic dots, 4 per lane); width 513 (16 per lane,
# five feature chunks of the gather, the last 1 wide); width 1024 -- and,
# independently of the shape, on att_dir (which launches run the softmax and
# its adjoint), on act (the logit and act') and on the mask (coef = alpha mask,
# dz = mask dalpha').  Pruning rule: the full att_dir x act x mask product at
# the botnet shape; every other shape once per att_dir, the acts and the mask
# rotating so that each shape meets a mask and two acts.  Soft and hard run
# every case (the hard structs change the logit and de in every kernel).
CASES = [(4, 8, d, a, m) for d in ("in", "out") for a in ("none", "relu", "lrelu")
         for m in (False, True)] + [
    (1, 7, "in", "lrelu", False), (1, 7, "out", "none", True),
    (3, 4, "in", "relu", True), (3, 4, "out", "lrelu", False),
    (8, 16, "in", "none", False), (8, 16, "out", "relu", True),
    (2, 128, "in", "lrelu", True), (2, 128, "out", "lrelu", False),
    (3, 171, "in", "lrelu", False), (3, 171, "out", "none", True),
    (16, 64, "in", "relu", False), (16, 64, "out", "lrelu", True),
]


def expected_calls(kind, adir):
    p = "mgcn_att" if kind == "soft" else "mgcn_hatt"
    exp = {p + "_fwd_sched": 1, p + "_bwd_dst_sched": 1, p + "_bwd_src_sched": 1}
    if adir == "out":
        exp[("mgcn_" if kind == "soft" else "mgcn_hatt_") + "edge_softmax_sched"] = 1
    return exp


@pytest.mark.parametrize("kind", ["soft", "hard"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_bits_equal_the_wave_path(cuda, kind, case):
    """Forward + backward with the route on and off: Y, alpha_coo, dHp and
    datt ``torch.equal``; the expected _sched entries ran once each in the
    first run and none in the second; a masked heavy group's alpha' is +0."""
    H, C, adir, act, mask = case
    runs, calls = {}, {True: {}, False: {}}
    for on in (True, False):
        with route(on, calls[on]):
            runs[on] = run_op(cuda, kind, H, C, adir, act, mask, seed=CASES.index(case))
    assert calls[True] == expected_calls(kind, adir) and calls[False] == {}
    for k, v in runs[True].items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, runs[False][k]), f"{k}: the heavy route changed bits"
    assert runs[True]["alpha_coo"].unique().numel() > 100
    if mask:
        ei, _, _ = hub_ladder(cuda)
        node, side = masked_group(adir)
        a0 = runs[True]["alpha_coo"][ei[side] == node]
        assert a0.shape == (513, H)
        assert torch.equal(a0.view(torch.int32), torch.zeros_like(a0, dtype=torch.int32))


@pytest.mark.parametrize("kind,adir", [("soft", "in"), ("hard", "out")])
def test_against_the_fp64_restatement(cuda, kind, adir):
    """Route on, against the plain-torch restatement in fp32 and fp64 under the
    attention tests' bound (attention_ref.check): catches a route wrong in the
    same way on and off."""
    H, C, act = 4, 8, "lrelu"
    ei, N, _ = hub_ladder(cuda)
    eic = ei.cpu()
    Hp, att, dY, noise, m = inputs(cuda, H, C, adir, True, 77)
    calls = {}
    with route(True, calls):
        got = run_op(cuda, kind, H, C, adir, act, True, seed=77)
    assert calls == expected_calls(kind, adir)
    ref = {}
    for dt in (torch.float32, torch.float64):
        x, a = (t.detach().clone().to(dt).requires_grad_(True) for t in (Hp, att))
        W = torch.eye(H * C, dtype=dt)
        if kind == "soft":
            y, alpha, _ = att_ref(x, W, a, None, eic, H, "cat", adir, act, m)
        else:
            y, alpha = hatt_ref(x, W, a, None, eic, H, "cat", adir, act, 0.5, True, noise, m)
        y.backward(dY.to(dt))
        ref[dt] = {"Y": y.detach(), "alpha_coo": alpha.detach(), "dHp": x.grad, "datt": a.grad}
    for k in ("Y", "alpha_coo", "dHp", "datt"):
        check(f"heavy.{kind}.{adir}.{k}", got[k], ref[torch.float32][k], ref[torch.float64][k])


@pytest.mark.parametrize("kind,adir", [("soft", "in"), ("soft", "out"), ("hard", "in"),
                                       ("hard", "out")])
def test_two_runs_are_bitwise_equal(cuda, kind, adir):
    with route(True):
        a = run_op(cuda, kind, 3, 171, adir, "lrelu", True, seed=5)
        b = run_op(cuda, kind, 3, 171, adir, "lrelu", True, seed=5)
    for k, v in a.items():
        assert torch.equal(v, b[k]), k


# ------------------------------------------------------------------ C ABI
PAD = 67  # guard elements on either side of a flat array


class Abi:
    """One forward + backward through the C entries of one kind and direction
    on the hub ladder, H = 3, C = 5."""
    H, C = 3, 5

    def __init__(self, cuda, kind, adir):
        import mgcn
        from mgcn import _lib as L
        self.L, self.lib, self.cuda, self.kind, self.adir = L, mgcn.load(), cuda, kind, adir
        _, self.N, self.plan = hub_ladder(cuda)
        N, nnz, H, C = self.N, self.plan.nnz, self.H, self.C
        gen = torch.Generator().manual_seed(8)
        rnd = lambda *s: torch.randn(*s, generator=gen).to(cuda)  # noqa: E731
        self.Hp, self.dY, self.att = rnd(N, H * C), rnd(N, H * C), rnd(H, 2 * C) * 0.5
        self.mask = ((torch.rand(nnz, H, generator=gen) < 0.5).float() * 2.0).to(cuda)
        self.noise = rnd(nnz, H)
        self.s_src = torch.empty(N, H, device=cuda)
        self.s_dst = torch.empty(N, H, device=cuda)
        L.check(self.lib.mgcn_att_scores(N, H, C, L.ptr(self.Hp), H * C, L.ptr(self.att),
                                         L.ptr(self.s_src), L.ptr(self.s_dst),
                                         L.stream_of(cuda)), "mgcn_att_scores")
        self.bufs = []  # (buffer, mask of the guard elements)

    def banded(self, *shape):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), float("nan"), device=self.cuda)
        m = torch.ones(n + 2 * PAD, dtype=torch.bool, device=self.cuda)
        m[PAD:PAD + n] = False
        self.bufs.append((buf, m))
        return buf[PAD:PAD + n].view(*shape)

    def window(self, ld, src=None):
        N, HC = self.N, self.H * self.C
        buf = torch.full((N + 2, ld), float("nan"), device=self.cuda)
        m = torch.ones_like(buf, dtype=torch.bool)
        m[1:N + 1, 2:2 + HC] = False
        self.bufs.append((buf, m))
        win = buf[1:N + 1, 2:2 + HC]
        if src is not None:
            win.copy_(src)
        return win

    def guards_ok(self):
        return all(bool(torch.isnan(buf[m]).all()) for buf, m in self.bufs)

    def entry(self, base, mode):
        hard = self.kind == "hard"
        if base == "edge_softmax":
            name = "mgcn_hatt_edge_softmax" if hard else "mgcn_edge_softmax"
        else:
            name = ("mgcn_hatt_" if hard else "mgcn_att_") + base
        return getattr(self.lib, name + ("" if mode == "old" else "_sched")), name

    def sched(self, mode, view, scratch, **bad):
        """The schedule arguments: none ('old'), order = NULL with a NULL coef
        ('null'), the view's schedule ('sched'); ``bad`` overrides."""
        if mode == "old":
            return ()
        given = mode == "sched"
        s = {"order": self.L.ptr(view.order) if given else None, "n_heavy": view.n_heavy,
             "n_giant": view.n_giant, "coef": self.L.ptr(scratch) if given else None}
        s.update(bad)
        tail = (s["order"], s["n_heavy"], s["n_giant"])
        return tail if scratch is None else tail + (s["coef"],)

    def run(self, mode, bad_entry=None, **bad):
        """mode 'old': the entries without a schedule; 'null': _sched with
        order = NULL; 'sched': the schedule, with rows as column windows and
        bands around every flat array.  ``bad_entry``: that entry gets the
        ``bad`` schedule arguments, must return MGCN_EINVAL and leave its
        outputs as they were; the run stops there."""
        L, lib, cuda, ptr = self.L, self.lib, self.cuda, self.L.ptr
        N, H, C, HC, nnz = self.N, self.H, self.C, self.H * self.C, self.plan.nnz
        fwd, bwd = self.plan.fwd, self.plan.bwd
        slot = self.plan.slot_map()
        st = L.stream_of(cuda)
        hard, inn = self.kind == "hard", self.adir == "in"
        T = (0.5,) if hard else ()
        wide = mode == "sched"
        flat = self.banded if wide else (
            lambda *s: torch.full(s, float("nan"), device=cuda))
        hp = self.window(HC + 3, self.Hp) if wide else self.Hp
        dy = self.window(HC + 11, self.dY) if wide else self.dY
        Y = self.window(HC + 11) if wide else flat(N, HC)
        dHp = self.window(HC + 3) if wide else flat(N, HC)
        alpha, a_bwd, dz, coef_f, coef_b = (flat(nnz, H) for _ in range(5))
        ds_src, ds_dst = flat(N, H), flat(N, H)
        act = 1  # lrelu

        def call(base, view, coef, outs, *args):
            fn, name = self.entry(base, mode)
            is_bad = bad_entry == base
            before = [o.clone() for o in outs]
            rc = fn(*args, *self.sched(mode, view, coef, **(bad if is_bad else {})), st)
            torch.cuda.synchronize()
            if is_bad:
                assert rc == L.EINVAL, (name, rc)
                for o, b in zip(outs, before):
                    assert torch.equal(o.view(torch.int32), b.view(torch.int32)), name
                return False
            assert rc == 0, lib.mgcn_last_error()
            return True

        noise_f = (ptr(self.noise),) + T if hard else ()
        if inn:
            if not call("fwd", fwd, coef_f, [Y, alpha], N, nnz, H, C, ptr(fwd.rowptr),
                        ptr(fwd.col), ptr(self.s_dst), ptr(self.s_src), act, *noise_f, None,
                        ptr(self.mask), ptr(hp), hp.stride(0), ptr(Y), Y.stride(0), ptr(alpha)):
                return None
        else:
            if not call("edge_softmax", bwd, None, [a_bwd], N, nnz, H, ptr(bwd.rowptr),
                        ptr(bwd.col), ptr(self.s_src), ptr(self.s_dst), act, *noise_f,
                        ptr(a_bwd)):
                return None
            alpha[slot[:nnz].long()] = a_bwd
            noise_n = (None,) + T if hard else ()
            if not call("fwd", fwd, coef_f, [Y], N, nnz, H, C, ptr(fwd.rowptr), ptr(fwd.col),
                        None, None, act, *noise_n, ptr(alpha), ptr(self.mask), ptr(hp),
                        hp.stride(0), ptr(Y), Y.stride(0), None):
                return None
        if not call("bwd_dst", fwd, None, [dz, ds_dst], N, nnz, H, C, ptr(fwd.rowptr),
                    ptr(fwd.col), ptr(hp), hp.stride(0), ptr(dy), dy.stride(0), ptr(alpha),
                    ptr(self.mask), ptr(self.s_dst), ptr(self.s_src), act, int(inn), *T, ptr(dz),
                    ptr(ds_dst)):
            return None
        if not call("bwd_src", bwd, coef_b, [dz, ds_src, dHp], N, nnz, H, C, ptr(bwd.rowptr),
                    ptr(bwd.col), ptr(slot), ptr(dy), dy.stride(0), ptr(alpha), ptr(self.mask),
                    ptr(dz), ptr(self.s_src), ptr(self.s_dst), act, int(not inn), *T,
                    ptr(self.att), ptr(ds_dst) if inn else None, ptr(ds_src), ptr(dHp),
                    dHp.stride(0)):
            return None
        out = {"Y": Y, "alpha": alpha, "dz": dz, "ds_src": ds_src, "dHp": dHp}
        if inn:
            out["ds_dst"] = ds_dst
        return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("adir", ["in", "out"])
@pytest.mark.parametrize("kind", ["soft", "hard"])
def test_c_abi_schedule_windows_and_guard_bands(cuda, kind, adir):
    """Every _sched entry called directly.  order = NULL (coef NULL): the bits
    of the entry without a schedule.  With the schedule, Hp / Y / dY / dHp as
    column windows (ld = H C + 3 / + 11) of NaN-filled buffers and NaN bands
    around alpha, dz, ds and the scratch: those bits again, every padding
    column and guard element intact.  A bad schedule or a missing scratch:
    MGCN_EINVAL, outputs untouched."""
    abi = Abi(cuda, kind, adir)
    old = abi.run("old")
    for k, v in old.items():
        assert not torch.isnan(v).any(), k
    for mode in ("null", "sched"):
        got = abi.run(mode)
        for k, v in old.items():
            assert torch.equal(got[k], v), f"{mode}: {k}"
    assert len(abi.bufs) == 11 and abi.guards_ok()
    N = abi.N
    entries = ["fwd", "bwd_dst", "bwd_src"] + (["edge_softmax"] if adir == "out" else [])
    for base in entries:
        assert abi.run("sched", base, n_giant=4, n_heavy=3) is None
        assert abi.run("sched", base, n_heavy=N + 1) is None
        if base in ("fwd", "bwd_src"):
            assert abi.run("sched", base, coef=None) is None


# ----------------------------------------------------------------- routing
def test_routing(cuda):
    """Which C entry runs: switch off -> no _sched entry; a graph with all
    degrees <= 128 -> none; bf16 rows -> none; hard eval routes its backward
    alone (the shared att_bwd_src)."""
    from mgcn.graph import plan_for
    from mgcn.ops import attention_aggregate, hard_attention_aggregate
    for kind in ("soft", "hard"):
        for adir in ("in", "out"):
            calls = {}
            with route(False, calls):
                run_op(cuda, kind, 2, 4, adir, "lrelu", False)
            assert calls == {}
            with route(True, calls):
                run_op(cuda, kind, 2, 4, adir, "lrelu", False, dtype=torch.bfloat16)
            assert calls == {}
    # no heavy rows: the ladder's pool alone (degrees < 128)
    gen = torch.Generator().manual_seed(3)
    N = 70
    ei = torch.randint(0, N, (2, 400), generator=gen).to(cuda)
    plan = plan_for(ei, N)
    assert plan.fwd.n_heavy == 0 and plan.bwd.n_heavy == 0
    Hp = torch.randn(N, 8, generator=gen).to(cuda).requires_grad_(True)
    att = torch.randn(1, 2, 8, generator=gen).to(cuda)
    calls = {}
    with route(True, calls):
        for adir in ("in", "out"):
            attention_aggregate(Hp, att, plan, 2, "lrelu", adir)[0].sum().backward()
            hard_attention_aggregate(Hp, att, plan, 2, "lrelu", adir, 0.5,
                                     training=True)[0].sum().backward()
    assert calls == {}
    # hard eval on the hub ladder: forward on the wave kernels, backward routed
    _, Nh, hplan = hub_ladder(cuda)
    Hp = torch.randn(Nh, 8, generator=gen).to(cuda).requires_grad_(True)
    res = {}
    for on in (True, False):
        calls = {}
        Hp.grad = None
        with route(on, calls):
            Y, _ = hard_attention_aggregate(Hp, att, hplan, 2, "lrelu", "in", training=False)
            assert calls == {}
            Y.backward(torch.ones_like(Y))
        assert calls == ({"mgcn_att_bwd_src_sched": 1} if on else {})
        res[on] = (Y.detach(), Hp.grad.clone())
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


def test_env_switch_in_a_fresh_process(cuda):
    """MGCN_ATT_HEAVY=0, read at import: no _sched entry runs on the ladder."""
    code = (
        "import sys, torch\n"
        "sys.path[:0] = %r\n"
        "import test_gpu_attention_heavy as t\n"
        "from mgcn import ops\n"
        "assert ops.attention_heavy_rows() is False\n"
        "calls = {}\n"
        "with t.route(ops.attention_heavy_rows(), calls):\n"
        "    t.run_op(torch.device('cuda:0'), 'soft', 2, 4, 'out', 'lrelu', False)\n"
        "assert calls == {}, calls\n"
        "print('ok')\n" % [p for p in sys.path if p])
    env = dict(os.environ, MGCN_ATT_HEAVY="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


# ------------------------------------------------------------------ models
def _model_run(cuda, which, on):
    from mgcn.models import GCNModel, NodeModelHardAttention
    ei, N, _ = hub_ladder(cuda)
    torch.manual_seed(3)
    if which == "gcn":
        m = GCNModel(6, [8, 8], 2, final_type='proj', nodemodel='attention', nheads=[2, 1],
                     att_dir='in').to(cuda)
    else:
        m = NodeModelHardAttention(6, 8, nheads=2, att_dir='in').to(cuda)
    m.train()
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(N, 6, generator=gen).to(cuda)
    calls = {}
    torch.manual_seed(11)  # dropout and the Gumbel noise draw the same numbers
    with route(on, calls):
        out = m(x, ei)
        dOut = torch.randn(out.shape, generator=gen).to(cuda)
        out.backward(dOut)
    torch.cuda.synchronize()
    res = {"out": out.detach()}
    for k, p in m.named_parameters():
        if p.grad is not None:  # (NodeModelBase keeps parameters attention does not use)
            res[k] = p.grad
    return res, calls


@pytest.mark.parametrize("which", ["gcn", "hard"])
def test_model_bits(cuda, which):
    """A 2-layer GCNModel(nodemodel='attention', nheads=[2, 1], att_dir='in')
    and a NodeModelHardAttention layer on the hub ladder: output and every
    parameter gradient ``torch.equal`` with the route on and off."""
    on, c_on = _model_run(cuda, which, True)
    off, c_off = _model_run(cuda, which, False)
    assert c_off == {} and c_on and all(k.endswith("_sched") for k in c_on)
    assert on.keys() == off.keys() and len(on) >= 3
    for k, v in on.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, off[k]), f"{k}: on != off"
