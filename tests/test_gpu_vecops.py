"""GPU: every Krylov vector and layout kernel of ``csrc/vecops.hip`` on its own, through the test hook ``mitdvp_vecop`` /
``engine.vecop`` (one call of the host wrapper, on a stream of its own, the wrapper's grid choice included), held to the
NumPy models of ``helpers.vecops_ref`` at the bars written next to them there.

The larger operations reach these kernels only at the sizes their fixtures happen to produce; here each meets a plain
reference above double precision at the shapes where it can go wrong: the 256-workgroup reductions below, at and above
their second grid-stride pass (65536 elements), consumers fed partials spread over all 256 entries, the one-workgroup
Lanczos step at every register slot up to 16384 and its refusal at 16385, the transpose on and around its 32 x 32 tile with
padding on either side and with interleaved batches, ``permute5`` in both Kraus forms, on a zero stride and past the 4096
workgroup cap, the block lists with repeats and an empty list, the norm profiles around 256 rows, and the identity tests with
NaN and +-Inf.  Results are in-out: every element outside the written set -- padding between ``cols`` and ``ld``, skipped
blocks, the guard elements behind the footprint -- must keep the NaN payload it was given.

One test per group of ``vecops_ref.CASES``, rows smallest first; under ``-s`` one line per row with the defect and its bar.

What the file found: no kernel missed its model.  ``phys_diag`` was the one wrapper without a zero-size return (a grid of 0
workgroups, which HIP refuses); it has one now and the zero-size rows run it.  With ``clear`` set, ``ident_deviation_multi``
zeroes the outputs of ALL blocks before it looks at the masked ones, so a block that was not asked for comes back as +0.0,
not as it was (its ``lam`` is left alone); the rows assert exactly that.  Run for the first time beyond one tile, one pass
or two register slots with a bar of their own: ``k_lanczos_step_small`` (slots 3 .. 16, the ragged last slot), the
``NPART``-grid kernels above 65536 elements (``k_dot``, ``k_sumsq``, ``k_lanczos_update``, ``k_lanczos_update_def``,
``k_multi_dot``, ``k_arnoldi_update``, ``k_lincomb``), ``k_transpose`` with padded leading dimensions and interleaved
batches beyond one tile, and the second pass of the four 4096-capped grids.

The largest bar of the table is 0.17, on the norm of the one-workgroup step at n = 16384: the bound of alpha, which holds
for any order of its 16384 terms, is carried through every element into the sum of squares (the defect there is 5e-11);
the lost element it must still show moves that sum by 0.25 at least.  ``test_the_one_workgroup_step_equals_the_three_kernels``
therefore also holds w and the norm to the model evaluated with the alpha the step returned, where that bound drops out: the
norm's bar is then its own reduction bar, 3e-6 at n = 16384.

Figures of one run on an MI355X: profiles/vecops_tests.txt.
"""

import numpy as np
import pytest

from helpers import vecops_ref as vr

pytestmark = pytest.mark.gpu


def run(row, g, **over):
    from pytdscf_amd import engine as E

    kw = dict(variant=row["variant"], z=g["z"], r=g["r"], idx=g["idx"], mask=g["mask"], zo=g["zo"], ro=g["ro"], a=g["a"], b=g["b"],
              both=g["both"], eps=g["eps"], coef=g["coef"], f=g["f"])
    kw.update(over)
    zo0, zo1, ro = E.vecop(row["op"], row["dims"], row["strides"], **kw)
    return dict(zo0=zo0, zo1=zo1, ro=ro)


@pytest.mark.parametrize("group", vr.GROUPS)
def test_rows_meet_their_models(group):
    rows = [r for r in vr.CASES if r["group"] == group]
    assert rows
    failed = []
    for r in rows:
        g = vr.build(r)
        got = run(r, g)
        line = []
        for key, spec in vr.expect(r, g).items():
            ok, defect, bar, what = vr.judge(spec, got[key])
            line.append(f"{key} {'bits' if bar == 0 and ok else f'{defect:.2e} / {bar:.2e}'}")
            if not ok:
                failed.append((r["name"], key, defect, bar, what))
        print(f"[vecops] {r['name']}: " + ", ".join(line))
    print(f"[vecops] {group}: {len(rows)} rows, {len(failed)} failed")
    assert not failed, failed[:5]


def test_the_one_workgroup_step_equals_the_three_kernels():
    """w, alpha and the norm of lanczos_step_small against dot + lanczos_update + scale_inv_norm through the hook on the
    same input, within the sum of the two bars: the step's own, and the same again for the three kernels plus the bound
    (NPART + 2) u sum|p| of the two partial arrays they pass on (alpha into the update, the norm into the scaling).
    Before that, w and the norm against the model evaluated with the alpha the step returned."""
    rows = [r for r in vr.CASES if r["op"] == "lanczos_step_small"]
    assert {r["dims"][0] for r in rows} == set(vr.SMALL_NS)
    for r in rows:
        g = vr.build(r)
        n, v = r["dims"][0], r["variant"]
        sp = vr.expect(r, g)
        small = run(r, g)
        # the update and the norm once more, from the alpha the step itself returned: the any-order bound of alpha drops
        # out, and the norm is held to its own reduction bar (3e-6 at n = 16384, where the table's bar is 0.17)
        own = vr.expect(r, dict(g, alpha_dev=small["zo1"][0]))
        for key in ("zo0", "ro"):
            ok, defect, bar, what = vr.judge(own[key], small[key])
            print(f"[vecops] {r['name']} from its own alpha: {key} {defect:.2e} / {bar:.2e}")
            assert ok, (r["name"], key, defect, bar, what)
        x = g["z"][1] if v & 2 else g["z"][0]
        dot = {"op": "dot", "dims": (n,), "strides": (), "variant": 1}
        alpha_p = run(dot, dict(g, z=[x, g["zo"][0][:n], None], zo=[vr.result(vr.NPART), None], ro=None, r=None))["zo0"]
        upd = {"op": "lanczos_update", "dims": (n,), "strides": (), "variant": v & 1}
        u = run(upd, dict(g, z=[g["z"][0], g["z"][2], alpha_p[:vr.NPART]], zo=[g["zo"][0], None], ro=vr.result(vr.NPART, cplx=False)))
        sc = {"op": "scale_inv_norm", "dims": (n,), "strides": (), "variant": 0}
        w3 = run(sc, dict(g, z=[None] * 3, r=u["ro"][:vr.NPART], zo=[u["zo0"], None], ro=None))["zo0"]
        pa = (vr.NPART + 2) * vr.U * float(np.abs(alpha_p[:vr.NPART]).sum())
        pn = (vr.NPART + 2) * vr.U * float(np.abs(u["ro"][:vr.NPART]).sum())
        s = float(sp["ro"]["ref"][0])
        inv = 1.0 / np.sqrt(s) if np.sqrt(s) >= g["eps"] else 1.0
        wref = np.abs(sp["zo0"]["ref"][:n]).astype(np.float64)
        tol_w = 2 * sp["zo0"]["bar"][:n] + 2 * pa * np.abs(g["z"][0]) * inv + wref * pn / (2 * s)
        tol_a, tol_n = 2 * float(sp["zo1"]["bar"][0]) + pa, 2 * float(sp["ro"]["bar"][0]) + pn
        dw = small["zo0"][:n] - w3[:n]
        dw = np.maximum(np.abs(dw.real), np.abs(dw.imag))
        da = abs(small["zo1"][0] - vr.xsum(alpha_p[:vr.NPART]))
        dn = abs(small["ro"][0] - vr.xsum(u["ro"][:vr.NPART]))
        j = int(np.argmax(dw / tol_w))
        print(f"[vecops] {r['name']} against the three kernels: w {dw[j]:.2e} / {tol_w[j]:.2e}, alpha {float(da):.2e} / {tol_a:.2e}, "
              f"norm {float(dn):.2e} / {tol_n:.2e}")
        assert np.all(dw <= tol_w) and da <= tol_a and dn <= tol_n, r["name"]
        assert np.array_equal(vr.bits(small["zo0"][n:]), vr.bits(w3[n:]))


def test_the_one_workgroup_step_refuses_a_longer_vector():
    from pytdscf_amd import engine as E

    n = vr.SMALL_VEC_N + 1
    w = np.ones(n, complex)
    with pytest.raises(ValueError, match="SMALL_VEC_N"):
        E.vecop("lanczos_step_small", (n,), z=[w, None, None], zo=[w, np.zeros(vr.NPART, complex)], ro=np.zeros(vr.NPART))


def test_the_shell_profile_sums_to_the_leading_blocks():
    """the header's identity |x[:D, :D]|^2 = sum_{t < D} out[t], at the sum of the shells' bars plus the block's own"""
    for r in (q for q in vr.CASES if q["op"] == "shell_sumsq"):
        g = vr.build(r)
        n = r["dims"][0]
        out, bar = run(r, g)["ro"][:n], vr.expect(r, g)["ro"]["bar"][:n]
        x = g["z"][0].reshape(n, n)
        worst = 0.0
        for D in sorted({1, n // 2, n - 1, n} - {0}):
            blk = np.abs(x[:D, :D]).astype(np.float64) ** 2
            defect = abs(float(vr.xsum(out[:D]) - vr.xsum(blk.reshape(-1))))
            tol = float(bar[:D].sum()) + (D + 4) * vr.U * float(blk.sum())
            worst = max(worst, defect / tol)
            assert defect <= tol, (r["name"], D, defect, tol)
        print(f"[vecops] {r['name']}: the leading blocks at {worst:.2f} of their bar")


def test_a_zero_size_call_leaves_the_results():
    """every wrapper with a zero-size return of its own is called with nothing to do (phys_diag had none: a grid of 0)"""
    from pytdscf_amd import engine as E

    keep = vr.sentinel(4)
    for op, dims, strides, variant in (
            ("phys_diag", (0, 3, 5), (), 0), ("phys_diag", (0, 3, 5), (), 1), ("phys_diag", (4, 0, 5), (), 0), ("phys_diag", (4, 3, 0), (), 1),
            ("copy2d", (0, 3, 0), (3, 3), 1), ("transpose", (0, 5, 2), (5, 1, 0, 0), 0), ("transpose_rev3", (3, 0, 2), (), 0),
            ("permute_0213", (2, 0, 3, 1), (), 0), ("copy_raw", (0,), (), 0), ("permute5", (1, 2, 0, 1, 1), (0, 0, 0, 0, 0), 0),
            ("scale_cols", (0, 4), (4,), 0), ("dot", (0,), (), 1)):
        zo0, _, _ = E.vecop(op, dims, strides, variant=variant, z=[keep, keep, None], r=np.ones(4), zo=[keep.copy(), None])
        assert np.array_equal(vr.bits(zo0), vr.bits(keep)), op
