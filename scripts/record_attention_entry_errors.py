"""Record what the 22 view-walking attention entries of libmgcn answer to
arguments they must refuse (or accept as a no-op) before any launch.

    python scripts/record_attention_entry_errors.py [--out tests/golden/attention_entry_errors.json]

The entries: soft and hard x fwd, edge_softmax, bwd_dst, bwd_src x plain,
_bf16, _sched (the edge softmax touches no feature row: no _bf16).  Every
pointer is a dummy that is never dereferenced (tests/test_attention_heavy_host.py):
a case either fails a host check (MGCN_EINVAL) or is one of the no-ops that
return MGCN_OK before a launch.  The script refuses to record anything else,
so no recorded case reaches a launch.  Run it on a machine without a device,
against the build of the commit whose answers are the yardstick; it writes
(entry, case) -> [return code, mgcn_last_error()].
tests/test_attention_entries_host.py replays cases() against the tree.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meta-gcn_amd")]

P = ctypes.c_void_p(0x1000)  # never dereferenced
H, C = 2, 4
OPS = ("fwd", "edge_softmax", "bwd_dst", "bwd_src")
# argument names in ABI order; {hard} / {sched} / {park} mark where the
# variants splice theirs in
ORDER = {
    "fwd": "n nnz H C rowptr col s_row s_col act {noise_T} alpha_in mask Hp ldh Y ldy alpha "
           "{sched} {coef}",
    "edge_softmax": "n nnz H rowptr col s_row s_col act {noise_T} alpha {sched}",
    "bwd_dst": "n nnz H C rowptr col Hp ldh dY lddy alpha mask s_row s_col act softmax {T} dz "
               "ds_row {sched}",
    "bwd_src": "n nnz H C rowptr col slot dY lddy alpha mask dz s_row s_col act softmax {T} a "
               "ds_dst ds_src dHp lddh {park} {sched} {coef}",
}
DEFAULTS = dict(n=4, nnz=6, H=H, C=C, act=1, softmax=1, T=0.5, ldh=H * C, ldy=H * C, lddy=H * C,
                lddh=H * C, alpha_in=None, mask=None, ds_dst=None, dHp_f32=None, n_heavy=1,
                n_giant=0)


def entries():
    """{entry: (op, hard, variant)} for the 22 entries."""
    out = {}
    for hard in (False, True):
        for op in OPS:
            base = "mgcn_" + ("hatt_" if hard else "" if op == "edge_softmax" else "att_") + op
            for variant in ("", "_bf16", "_sched"):
                if op == "edge_softmax" and variant == "_bf16":
                    continue
                out[base + variant] = (op, hard, variant)
    return out


def arguments(op, hard, variant, **kw):
    """The ctypes argument tuple of an entry: DEFAULTS (a call that would pass
    every check), every other argument the dummy pointer, overridden by kw."""
    sched = variant == "_sched"
    names = ORDER[op].format(noise_T="noise T" if hard else "", T="T" if hard else "",
                             park="dHp_f32" if variant == "_bf16" else "",
                             sched="order n_heavy n_giant" if sched else "",
                             coef="coef" if sched else "").split()
    unknown = set(kw) - set(names)
    assert not unknown, (op, hard, variant, unknown)
    vals = dict(DEFAULTS)
    vals.update(kw)
    return tuple(vals.get(k, P) for k in names) + (None,)  # the stream


def op_cases(op, hard, variant):
    """{case: (overrides, is a listed no-op)} of one entry."""
    gather = op != "edge_softmax"
    sched = variant == "_sched"
    cs = {}

    def bad(name, **kw):
        cs[name] = (kw, False)

    def noop(name, **kw):
        cs[name] = (kw, True)

    bad("negative_n_rows", n=-1)
    bad("negative_nnz", nnz=-1)
    bad("H_0", H=0)
    bad("H_17", H=17)
    if gather:
        bad("HC_1025", H=1, C=1025)
        bad("C_0", C=0)
    bad("nnzH_2p31", nnz=2 ** 30)
    bad("act_3", act=3)
    bad("act_negative", act=-1)
    bad("shape_before_act", H=0, act=3)
    if hard:
        bad("temperature_0", T=0.0)
        bad("temperature_negative", T=-1.0)
        bad("temperature_before_n_rows_0", T=0.0, n=0, nnz=0)
        bad("act_before_temperature", act=3, T=0.0)
    noop("n_rows_0", n=0, nnz=0, **(dict(n_heavy=0) if sched else {}))
    bad("null_rowptr", rowptr=None)
    bad("null_col", col=None)
    if op == "edge_softmax":
        noop("nnz_0", nnz=0)
        noop("nnz_0_before_null_check", nnz=0, rowptr=None, col=None, s_row=None, s_col=None,
             alpha=None)
        noop("n_rows_0_before_null_check", n=0, nnz=0, rowptr=None, alpha=None,
             **(dict(n_heavy=0) if sched else {}))
        for k in ("s_row", "s_col", "alpha"):
            bad("null_" + k, **{k: None})
    if op == "fwd":
        bad("null_Hp", Hp=None)
        bad("null_Y", Y=None)
        bad("null_before_null_col", Y=None, col=None)
        bad("no_alpha_in_no_s_row", s_row=None)
        bad("no_alpha_in_no_s_col", s_col=None)
        bad("no_alpha_in_no_alpha", alpha=None)
        bad("ldh_small", ldh=H * C - 1)
        bad("ldy_small", ldy=H * C - 1)
        bad("alpha_in_ldh_small", alpha_in=P, s_row=None, s_col=None, alpha=None, ldh=H * C - 1)
    if op == "bwd_dst":
        bad("null_Hp", Hp=None)
        bad("null_dY", dY=None)
        bad("null_dz", dz=None)
        for k in ("alpha", "s_row", "s_col", "ds_row"):
            bad("softmax_needs_" + k, **{k: None})
        bad("no_softmax_ldh_small", softmax=0, alpha=None, s_row=None, s_col=None, ds_row=None,
            ldh=H * C - 1)
        bad("ldh_small", ldh=H * C - 1)
        bad("lddy_small", lddy=H * C - 1)
    if op == "bwd_src":
        for k in ("dY", "a", "ds_src"):
            bad("null_" + k, **{k: None})
        for k in ("slot", "alpha", "dz"):
            bad("null_" + k, **{k: None})
        bad("softmax_needs_s_row", s_row=None)
        bad("softmax_needs_s_col", s_col=None)
        bad("null_dHp", dHp=None)
        bad("no_softmax_null_dHp", softmax=0, s_row=None, s_col=None, dHp=None)
        bad("lddy_small", lddy=H * C - 1)
        bad("lddh_small", lddh=H * C - 1)
        if variant == "_bf16":
            # a parked row makes a null dHp legal: recorded only where n_rows = 0
            # returns before it
            noop("parked_null_dHp_n_rows_0", n=0, nnz=0, dHp=None, dHp_f32=P)
            bad("parked_lddy_small", dHp=None, dHp_f32=P, lddy=H * C - 1)
            bad("parked_null_ds_src", dHp=None, dHp_f32=P, ds_src=None)
    if sched:
        bad("sched_n_giant_above_n_heavy", n_heavy=2, n_giant=3)
        bad("sched_n_heavy_above_n_rows", n_heavy=5)
        bad("sched_n_giant_negative", n_giant=-1)
        bad("sched_before_n_rows_0", n=0, nnz=0, n_heavy=1)
        bad("act_before_sched", act=3, n_heavy=5)
        bad("sched_before_null_check", n_heavy=5, rowptr=None)
        if hard:
            bad("temperature_before_sched", T=0.0, n_heavy=5)
        if op in ("fwd", "bwd_src"):
            bad("missing_coef", coef=None)
            bad("null_before_missing_coef", coef=None, rowptr=None)
            noop("order_null_n_rows_0", n=0, nnz=0, order=None, n_heavy=7, n_giant=9, coef=None)
            bad("order_null_needs_no_coef", order=None, n_heavy=7, n_giant=9, coef=None, H=17)
        else:
            noop("order_null_n_rows_0", n=0, nnz=0, order=None, n_heavy=7, n_giant=9)
            bad("order_null_counts_not_read", order=None, n_heavy=7, n_giant=9, H=17)
        bad("order_null_sibling_name", order=None, rowptr=None)
        if op == "edge_softmax":
            bad("sched_before_nnz_0", nnz=0, n_heavy=5)
    return cs


def cases():
    """{entry: {case: (ctypes arguments, is a listed no-op)}}"""
    return {name: {c: (arguments(*key, **kw), ok) for c, (kw, ok) in op_cases(*key).items()}
            for name, key in entries().items()}


def call(lib, entry, args):
    rc = getattr(lib, entry)(*args)
    return [rc, lib.mgcn_last_error().decode()]


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden",
                                                  "attention_entry_errors.json"))
    args = ap.parse_args()
    import torch

    import mgcn
    from mgcn import _lib as L
    assert not torch.cuda.is_available(), "record where no device exists: pointers are dummies"
    lib = mgcn.load()
    out = {}
    for entry, table in cases().items():
        out[entry] = {}
        for case, (cargs, is_noop) in table.items():
            rc, err = call(lib, entry, cargs)
            if not (rc == L.EINVAL or (rc == L.OK and is_noop)):
                sys.exit(f"{entry} / {case}: returned {rc} ({err!r}): not MGCN_EINVAL and not a "
                         "listed no-op, so the call got past the host checks; not recorded")
            out[entry][case] = [rc, err]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:  # one case per line
        f.write("{\n" + ",\n".join(
            " %s: {\n%s\n }" % (json.dumps(e), ",\n".join(
                "  %s: %s" % (json.dumps(c), json.dumps(v)) for c, v in sorted(t.items())))
            for e, t in sorted(out.items())) + "\n}\n")
    print(f"{len(out)} entries, {sum(len(v) for v in out.values())} cases -> {args.out}")


if __name__ == "__main__":
    main()
