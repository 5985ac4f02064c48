"""GPU: the reducing epilogue of the MFMA zgemm over all thirteen of its bodies (``mitdvp_zgemm_reduce``) against the NumPy
model ``helpers.zgemm_reduce_ref``.

Every row of ``CASES`` names the body it must reach in the default setting, with the unguarded 4 x 4 x 4 variant off and
with the 4 x 4 x 4 form off; the hook reports the body it ran and the tests assert it (on a device whose 4 x 4 x 4 lane map
does not verify, against the row's expectation for that form off).  Each row runs at three geometries -- one (u, v) group,
exactly one 64 x 64 tile, a partial last tile in both directions -- behind the NN or the NT K loop, in the 4M and the 3M
product, writing and accumulating, with K in {1, 5, 16, 33}, in canary buffers: NaN around A, B and the core, a finite
sentinel around C, NaN in the owned part of C when the call overwrites.

Integer-valued cases (parts in [-2, 2]) are exact in any summation order in both product forms, so the WHOLE returned
buffer must equal the model bit for bit.  One Gaussian case per body and product form is held to
max|out - ref| < 1e-12 max|ref| against the model in extended precision -- the bar tests/test_gpu_edge_apply.py holds this
kernel to, for sums of these lengths -- with everything outside the owned part bitwise unchanged and a second call bitwise
the first.  Two engine cases run the edge apply at a bond dimension (41) whose (u, v) groups do not fill the last tile,
at the two shapes that take the unguarded bodies.

Figures of one run on an MI355X: profiles/zgemm_reduce_tests.txt.
"""

import ctypes as C
import time

import numpy as np
import pytest

from helpers import zgemm_reduce_ref as rr

pytestmark = pytest.mark.gpu

MODES = (0, 1)
BAR = 1e-12
STATS = {}  # body -> [kernel cases, worst Gaussian defect]
T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for body, (calls, worst) in sorted(STATS.items()):
        print(f"\n[zgemm_reduce] body {body}: {calls} kernel cases, worst Gaussian defect {worst:.3e} (bar {BAR:.0e})")
    print(f"\n[zgemm_reduce] module wall time {time.time() - T0:.1f} s")


def note(body, calls=0, defect=0.0):
    s = STATS.setdefault(body, [0, 0.0])
    s[0] += calls
    s[1] = max(s[1], defect)


@pytest.fixture(scope="module")
def forms():
    """which forms this device and process run: a shape that takes the 4 x 4 x 4 form wherever it is available, and one that
    takes its unguarded variant wherever that is on"""
    from pytdscf_amd import engine as E

    got = {}
    for name, (xm, yn, di) in (("b4", (8, 8, 3)), ("full", (16, 32, 16))):
        a = rr.layout(xm, yn, di, nu=1, nv=1, k=1)
        A, B, W, C0 = rr.make_case(a, np.random.default_rng(0), "int")
        got[name] = E.zgemm_reduce(a, A, B, W, C0)[1]
    assert got["b4"] in (7, 13) and got["full"] in (1, 4, 8), got
    out = {"b4": got["b4"] == 7, "full": got["full"] == 1}
    print(f"\n[zgemm_reduce] 4 x 4 x 4 form available: {out['b4']}, unguarded variant on: {out['full']}")
    return out


def expected_body(r, setting, forms):
    if not forms["b4"]:
        return r["expect"]["b4_off"]
    if setting == "default" and not forms["full"]:
        return r["expect"]["full_off"]
    return r["expect"][setting]


def compare(out, ref, a, kind, what):
    """int: the whole buffer bit for bit; gauss: everything the operation does not own bit for bit, the owned part at the
    bar.  Returns the Gaussian defect max|out - ref| / max|ref|."""
    own = rr.owned_c(a)
    if kind == "int":
        same = (out == ref) | (np.isnan(out) & np.isnan(ref))
        if not same.all():
            bad = np.flatnonzero(~same)
            inside = np.isin(bad, own)
            raise AssertionError(f"{what}: {bad.size} elements differ from the model ({(~inside).sum()} of them outside the owned "
                                 f"part), first at flat index {bad[0]} ({'inside' if inside[0] else 'OUTSIDE'} the owned part): "
                                 f"{out[bad[0]]} vs {ref[bad[0]]}")
        assert not np.isnan(out[own]).any(), f"{what}: NaN in the owned part of C"
        return 0.0
    rest = np.ones(out.size, bool)
    rest[own] = False
    if not np.array_equal(out[rest], ref[rest]):
        bad = np.flatnonzero(rest & (out != ref))
        raise AssertionError(f"{what}: {bad.size} elements OUTSIDE the owned part of C changed, first at flat index {bad[0]}: "
                             f"{out[bad[0]]} vs {ref[bad[0]]}")
    assert not np.isnan(out[own]).any(), f"{what}: NaN in the owned part of C -- pad was read, or C was not overwritten"
    dev = np.abs(out[own] - ref[own])
    err = dev.max() / np.abs(ref[own]).max()
    print(f"[zgemm_reduce] {what}: defect {err:.3e} (bar {BAR:.0e})")
    assert err < BAR, f"{what}: {err:.3e} >= {BAR:.0e}, worst at flat index {own[dev.argmax()]} (inside the owned part)"
    return err


def describe(r, a, setting, mode, body, kind):
    return (f"body {body} row {r['name']} (xm, yn, di) = ({a['xm']}, {a['yn']}, {a['di']}) {'NT' if a['transB'] else 'NN'} "
            f"{'3M' if mode else '4M'} setting {setting} acc={a['acc']} groups {a['m'] // a['xm']} x {a['n'] // a['yn']} K={a['k']} "
            f"C layout {r['c_layout']} {kind}")


@pytest.mark.parametrize("idx", range(len(rr.CASES)), ids=[r["name"] for r in rr.CASES])
def test_integer_cases_equal_the_model_bit_for_bit(idx, forms):
    from pytdscf_amd import engine as E

    r = rr.CASES[idx]
    for gi, geo in enumerate(rr.geometries(idx)):
        for acc in (0, 1):
            a = rr.layout(**geo, acc=acc)
            A, B, W, C0 = rr.make_case(a, np.random.default_rng(1000 * idx + 10 * gi + acc), "int")
            ref = rr.apply(a, A, B, W, C0)
            for setting in rr.settings_of(r):
                body = expected_body(r, setting, forms)
                for mode in MODES:
                    what = describe(r, a, setting, mode, body, "int")
                    out, variant = E.zgemm_reduce(dict(a, mode3m=mode, **rr.SETTINGS[setting]), A, B, W, C0)
                    assert variant == body, f"{what}: the call ran body {variant}"
                    compare(out, ref, a, "int", what)
                    note(body, 1)


def gauss_row(body, forms):
    """the first row, and the setting, that reach a body on this device (None: the body cannot run here)"""
    for setting in rr.SETTINGS:
        for idx, r in enumerate(rr.CASES):
            if setting in rr.settings_of(r) and expected_body(r, setting, forms) == body:
                return idx, setting
    return None


@pytest.mark.parametrize("mode", MODES, ids=["4M", "3M"])
@pytest.mark.parametrize("body", range(1, 14))
def test_gaussian_case_per_body_at_the_bar_and_repeatable(body, mode, forms):
    from pytdscf_amd import engine as E

    hit = gauss_row(body, forms)
    if hit is None:  # only where the device does not run the 4 x 4 x 4 form (bodies 1-7) or its unguarded variant (1, 2)
        assert body <= 7 and not (forms["b4"] and forms["full"]), body
        return
    idx, setting = hit
    r = rr.CASES[idx]
    a = rr.layout(**rr.geometries(idx)[2], acc=body % 2)
    A, B, W, C0 = rr.make_case(a, np.random.default_rng(77 * body + mode), "gauss")
    ref = rr.apply(a, A, B, W, C0, dtype=np.clongdouble)
    what = describe(r, a, setting, mode, body, "gauss")
    d = dict(a, mode3m=mode, **rr.SETTINGS[setting])
    out, variant = E.zgemm_reduce(d, A, B, W, C0)
    assert variant == body, f"{what}: the call ran body {variant}"
    err = compare(out, ref, a, "gauss", what)
    again, _ = E.zgemm_reduce(d, A, B, W, C0)
    assert np.array_equal(out, again), f"{what}: a second call differs bitwise, first at flat index {np.flatnonzero(out != again)[0]}"
    note(body, 2, err)


def test_default_product_form_is_one_of_the_two():
    """mode3m = -1 takes the library's default form: bitwise one of the two explicit ones"""
    from pytdscf_amd import engine as E

    a = rr.layout(12, 10, 12, nu=6, nv=7, k=33, transB=1, acc=1, pad=(1, 2, 3), off=(1, 2, 3, 4))
    A, B, W, C0 = rr.make_case(a, np.random.default_rng(5), "gauss")
    outs = {m: E.zgemm_reduce(dict(a, mode3m=m), A, B, W, C0)[0] for m in (-1, 0, 1)}
    assert np.array_equal(outs[-1], outs[1 if E.get_gemm_mode() == "3m" else 0])


def test_a_bad_descriptor_is_refused_and_leaves_c_untouched():
    from pytdscf_amd import _lib
    from pytdscf_amd import engine as E

    a = rr.layout(16, 32, 16, nu=5, nv=5, k=33, transB=1, acc=1, off=(1, 2, 3, 4))
    A, B, W, C0 = rr.make_case(a, np.random.default_rng(6), "int")
    ref = rr.apply(a, A, B, W, C0)
    out, variant = E.zgemm_reduce(a, A, B, W, C0)
    assert np.array_equal(out, ref) and variant in (1, 4, 8)
    last = rr.last_elements(a)
    bad = {
        "C one element short": (a, dict(C=last["C"])),
        "A one element short": (a, dict(A=last["A"])),
        "B one element short": (a, dict(B=last["B"])),
        "W one element short": (a, dict(W=last["W"])),
        "m no multiple of xm": (dict(a, m=a["m"] - 1), {}),
        "n no multiple of yn": (dict(a, n=a["n"] - 1), {}),
        "shape not served": (dict(a, xm=8, yn=8, di=17), {}),
        "negative stride": (dict(a, sv=-1), {}),
        "negative offset": (dict(a, offW=-1), {}),
        "epi_b4 = 1": (dict(a, epi_b4=1), {}),
        "epi_full = 1": (dict(a, epi_full=1), {}),
    }
    for what, (d, sizes) in bad.items():
        s = _lib.ZgemmReduceArgs()
        for name, val in rr.full(d).items():
            setattr(s, name, int(val))
        Cb = C0.copy()
        n = {"A": A.size, "B": B.size, "W": W.size, "C": Cb.size}
        n.update(sizes)
        v = C.c_int(-7)
        rc = _lib.load().mitdvp_zgemm_reduce(0, C.byref(s), E._dp(A), n["A"], E._dp(B), n["B"], E._dp(W), n["W"], E._dp(Cb), n["C"],
                                              C.byref(v))
        assert rc == _lib.EINVAL and v.value == -7, (what, rc, v.value)
        assert np.array_equal(Cb, C0, equal_nan=True), f"{what}: a refused call changed C"
    # nothing to do: success, C as it came
    for d in (dict(a, m=0), dict(a, n=0)):
        out, variant = E.zgemm_reduce(d, A, B, W, C0)
        assert np.array_equal(out, C0, equal_nan=True) and variant == 0


@pytest.mark.parametrize("d,M,body", [(16, 32, 1), (32, 16, 2)])
def test_engine_edge_apply_with_a_partial_last_tile(d, M, body, forms):
    """The call the hook exercises is the call the engine makes: a six-site chain with bond dimension 41 -- the (u, v)
    groups of either side then do not fill the last tile -- at the two (d, M) whose sides run the unguarded bodies, in
    the edge form with neither side folded, against the oracle's plain contraction."""
    from helpers import fold_seam as fs
    from oracle import tdvp_oracle as orc
    from pytdscf_amd import synthetic as syn

    L, D, c = 6, 41, 2
    for r in rr.CASES:  # both sides of this site run the body named (where the device runs it at all)
        if r["name"] in (f"d{d}M{M}-R", f"d{d}M{M}-L"):
            assert r["expect"]["default"] == body and (r["xm"], r["yn"], r["di"]) == ((d, M, d) if r["transB"] else (M, d, d))
    assert D % (64 // d) and D % (64 // M)
    mpo = syn.synthetic_mpo(L, d, M, seed=0)
    eng = fs.engine_under(L, {"MITDVP_EDGE_APPLY": "1", "MITDVP_FOLD_APPLY": "0"})
    try:
        eng.set_mpo(mpo)
        eng.init_random([d] * L, D, seed=1)
        assert eng.get_site_shape(c)[:3] == (D, d, D)
        fs.to_site(eng, c)
        fs.check_center(orc, eng, mpo, c, np.random.default_rng(100 + d), fs.EDGE)  # bit 0x10 set, 0x20 and 0x40 clear
    finally:
        eng.close()
