"""CPU-only checks of the seeded edge-noise generator's host side (no GPU
compute): the numpy restatement against Random123's known answers, the C
entry's argument answers, the seed draw, and the modules' ``edge_rng``."""
import numpy as np
import pytest
import torch

import philox_ref as pr

# Random123 kat_vectors, philox4x32 with 10 rounds: counter, key -> output
KAT = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000",
     "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff",
     "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0",
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def _words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_restatement_reproduces_the_known_answers(ctr, key, out):
    got = pr.philox4x32_10(np.array(_words(ctr), dtype=np.uint32), _words(key))
    assert [int(w) for w in got] == _words(out)


def test_restatement_counter_layout_and_u():
    """uniform() is the definition: word h % 4 of the call with counter
    (e, h / 4, offset lo, offset hi) under key (seed lo, seed hi)."""
    seed, offset = 0xfedcba9876543210 >> 1, 2 ** 32 + 5
    eid = np.array([7, 0, 2 ** 31 - 1, 3], dtype=np.int32)
    u = pr.uniform(seed, offset, 4, 6, eid)
    assert u.dtype == np.float32 and u.shape == (4, 6)
    for k, e in enumerate(eid):
        for h in range(6):
            w = pr.philox4x32_10(np.array([e, h // 4, 5, 1], dtype=np.uint32),
                                 (seed & 0xffffffff, seed >> 32))[h % 4]
            assert u[k, h] == np.float32(int(w) >> 8) * np.float32(2.0 ** -24)
    assert 0.0 <= u.min() and u.max() <= 1.0 - 2.0 ** -24
    np.testing.assert_array_equal(pr.uniform(seed, offset, 3, 6), pr.uniform(
        seed, offset, 3, 6, np.arange(3)))
    # the transforms' extremes: finite for every u, the two special p exact
    g = pr.gumbel32(np.array([0.0, 1.0 - 2.0 ** -24], dtype=np.float32))
    assert np.isfinite(g).all() and -3.85 < g[0] < -3.82 and 16.6 < g[1] < 16.7
    assert (pr.dropout32(u, 0.0) == 1.0).all() and (pr.dropout32(u, 1.0) == 0.0).all()


def test_entry_answers_without_a_device():
    """mgcn_edge_noise answers from its argument checks alone, before any HIP
    call: 0 for nnz == 0, MGCN_EINVAL for every unsupported argument."""
    import mgcn
    from mgcn import _lib as L
    lib = mgcn.load()
    U, G, D = L.NOISE_UNIFORM, L.NOISE_GUMBEL, L.NOISE_DROPOUT
    assert (U, G, D) == (0, 1, 2)

    def call(kind, nnz, H, p=0.0, out=None):
        return lib.mgcn_edge_noise(kind, 1, 2, nnz, H, None, p, out, None)

    for kind in (U, G, D):
        assert call(kind, 0, 4, 0.5) == L.OK
    # a non-NULL out that must never be written (the checks come first)
    out = torch.full((4,), 7.0)
    bad = [call(G, 1, 0, out=out.data_ptr()), call(G, 1, 17, out=out.data_ptr()),
           call(U, 2 ** 27, 16, out=out.data_ptr()), call(3, 1, 1, out=out.data_ptr()),
           call(-1, 1, 1, out=out.data_ptr()), call(G, -1, 1, out=out.data_ptr()),
           call(D, 1, 1, -0.1, out=out.data_ptr()), call(D, 1, 1, 1.5, out=out.data_ptr()),
           call(D, 1, 1, float("nan"), out=out.data_ptr()), call(G, 1, 1, out=None)]
    assert bad == [L.EINVAL] * len(bad)
    assert (out == 7.0).all()
    assert b"mgcn_edge_noise" in lib.mgcn_last_error()
    # p is read by DROPOUT alone: the other kinds take any value (nnz == 0: no launch)
    assert call(G, 0, 1, float("nan")) == L.OK and call(U, 0, 1, 9.0) == L.OK


def test_draw_edge_seed_replays_differs_and_stays_on_the_host(monkeypatch):
    from mgcn import ops

    def no_device(*a, **k):
        raise AssertionError("draw_edge_seed touched the device")
    monkeypatch.setattr(torch.cuda, "_lazy_init", no_device)
    monkeypatch.setattr(torch.cuda, "synchronize", no_device)
    torch.manual_seed(1234)
    a1, a2 = ops.draw_edge_seed(), ops.draw_edge_seed()
    torch.manual_seed(1234)
    b1, b2 = ops.draw_edge_seed(), ops.draw_edge_seed()
    assert a1 == b1 and a2 == b2 and a1 != a2
    for pair in (a1, a2):
        assert len(pair) == 2 and all(type(v) is int and 0 <= v < 2 ** 63 for v in pair)
    # an explicit generator: its own stream, the global one untouched
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(1234)
    c = ops.draw_edge_seed(g)
    assert ops.draw_edge_seed() == a1 and c != a1
    assert ops.draw_edge_seed(torch.Generator().manual_seed(5)) == c


def test_descriptors_are_immutable_and_checked():
    import mgcn
    g = mgcn.DeviceGumbel(3, 4)
    d = mgcn.DeviceDropout(0.5, 3, 4)
    assert (g.seed, g.offset, d.p, d.seed, d.offset) == (3, 4, 0.5, 3, 4)
    with pytest.raises(Exception):
        g.seed = 5
    with pytest.raises(Exception):
        d.p = 0.1
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            mgcn.DeviceDropout(bad, 1, 2)
    with pytest.raises(ValueError):
        mgcn.DeviceGumbel(-1, 0)
    with pytest.raises(ValueError):
        mgcn.DeviceGumbel(0, 2 ** 63)
    assert mgcn.ops.edge_noise is mgcn.edge_noise and mgcn.ops.DeviceGumbel is mgcn.DeviceGumbel


def _modules(**kw):
    from mgcn.models import NodeModelAttention, NodeModelHardAttention
    from mgcn.votepool import VotePoolLayer
    return [NodeModelAttention(5, 12, nheads=3, att_dropout=0.5, **kw),
            NodeModelHardAttention(5, 12, nheads=3, att_dropout=0.5, **kw),
            VotePoolLayer(5, 12, nheads=3, att_dropout=0.5, **kw)]


def test_edge_rng_values_repr_and_state_dict():
    from mgcn.models import GCNModel, NodeModelAttention, NodeModelHardAttention
    from mgcn.votepool import VotePoolLayer, VotePoolModel
    for cls in (NodeModelAttention, NodeModelHardAttention, VotePoolLayer):
        with pytest.raises(ValueError, match="edge_rng"):
            cls(5, 12, nheads=3, edge_rng='bad')
    torch.manual_seed(0)
    default = _modules()
    torch.manual_seed(0)
    device = _modules(edge_rng='device')
    torch.manual_seed(0)
    explicit = _modules(edge_rng='torch')
    for a, b, c in zip(default, device, explicit):
        assert (a.edge_rng, b.edge_rng, c.edge_rng) == ('torch', 'device', 'torch')
        assert repr(a) == repr(b) == repr(c)
        assert list(a.state_dict()) == list(b.state_dict())
    # the keyword reaches the node models through the containers' **kwargs
    m = GCNModel(6, [8, 8], 3, nodemodel='attention', nheads=2, att_dropout=0.5,
                 edge_rng='device')
    assert all(layer.gcn.node_models[0].edge_rng == 'device' for layer in m.gcn_net)
    v = VotePoolModel(6, [8, 8], 3, nheads=2, edge_rng='device')
    assert all(net.edge_rng == 'device' for net in v.gpool_net)
    with pytest.raises(ValueError, match="edge_rng"):
        VotePoolModel(6, [8], 3, edge_rng='cpu')
    GCNModel(6, [8, 8], 3, edge_rng='device')  # additive node models take and ignore it
