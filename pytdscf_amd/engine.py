"""Thin Python handle over the C ABI (``include/mitdvp.h``).

Mirrors what ``WFunc``/``MPSCoefMPO`` expose for the hot path in the reference:
``propagate`` (= ``MPSCoef.propagate``, _mps_cls.py:452-503), ``expectation``,
``autocorr``, ``norm`` (_mps_cls.py:540-716).  Arrays are complex128, C order.
"""

from __future__ import annotations

import ctypes as C
import operator

import numpy as np

from . import _lib


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _c128(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.complex128))


def _is_dev(x) -> bool:
    """a torch tensor living on a GPU (complex128): handed to the library as a device pointer"""
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


class _Operand:
    """What a setter passes down: a host array (NumPy) or a device tensor (torch, complex128, contiguous).
    ``mode`` is the pointer mode the call needs (include/mitdvp.h, mitdvp_set_pointer_mode)."""

    def __init__(self, x):
        if _is_dev(x):
            import torch

            if x.dtype != torch.complex128:
                raise TypeError("device operands must be complex128")
            self.keep = x.contiguous()
            self.shape = tuple(self.keep.shape)
            self.ptr = C.cast(C.c_void_p(self.keep.data_ptr()), C.POINTER(C.c_double))
            self.mode = 1
        else:
            self.keep = _c128(x)
            self.shape = self.keep.shape
            self.ptr = _dp(self.keep)
            self.mode = 0
        self.ndim = len(self.shape)


class TDVPEngine:
    def __init__(
        self,
        nsite: int,
        *,
        device: int = 0,
        integrator: str = "lanczos",
        conserve_norm: bool = True,
        relax: bool | str = False,
        thresh: float = 1e-9,
        max_krylov: int = 20,
        lanczos_variant: str = "reference",
        cu_range: tuple[int, int] | None = None,
        max_diag_krylov: int = 0,
    ):
        """``max_diag_krylov``: the most Krylov vectors one local solve of ``relax="improved"`` may take (0: the library's
        default, 64; a solve that needs more raises "Lanczos Diagonalization is not converged in N basis").
        ``cu_range = (first, count)``: confine the engine to ``count`` compute units starting at ``first`` (multiples of 8:
        8 k units are k CUs on every XCD); engines with disjoint ranges never compete for a compute unit (TDVPEnsemble)."""
        lib = _lib.load()
        cfg = _lib.Config()
        cfg.nsite = nsite
        cfg.device = device
        cfg.integrator = {"lanczos": _lib.LANCZOS, "arnoldi": _lib.ARNOLDI}[integrator]
        cfg.conserve_norm = int(bool(conserve_norm))
        cfg.relax = 2 if relax == "improved" else int(bool(relax))
        cfg.thresh = thresh
        cfg.max_krylov = max_krylov
        cfg.lanczos_variant = {"reference": 0, "orthodox": 1}[lanczos_variant]
        cfg.max_diag_krylov = int(max_diag_krylov)
        if cu_range is not None:
            cfg.cu_first, cfg.cu_count = int(cu_range[0]), int(cu_range[1])
        self._lib = lib
        self._h = C.c_void_p()
        self.nsite = nsite
        self.device = device
        _lib.check(lib.mitdvp_create(C.byref(cfg), C.byref(self._h)))

    @classmethod
    def borrow(cls, handle, nsite: int, device: int):
        """Wrap an engine handle that something else owns (``mitdvp_shard_engine``): ``close`` only forgets it."""
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self._h = handle
        self._borrowed = True
        self.nsite = nsite
        self.device = device
        return self

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            if not getattr(self, "_borrowed", False):
                self._lib.mitdvp_destroy(self._h)
            self._h = None

    def heff_apply_center(self, x=None):
        """sigma = H_eff x at the centre site, through the very kernels a local exponential uses; returns
        (sigma, flags): bit 0 / 1 identity block of the left / right environment short-circuited, bit 2 block-sparse
        W stage, bit 3 one-launch small-bond kernel, 0x10 the edge form, 0x20 / 0x40 its R / L side folded, 0x80 / 0x100
        that folded R / L side as seven half-size products, 0x200 / 0x400 (with 0x80 / 0x100) each of those seven as seven
        quarter-size products."""
        c = next(p for p in range(self.nsite) if self.get_site_shape(p)[3] == _lib.GAUGE_PSI)
        l, n, r, _ = self.get_site_shape(c)
        out = np.empty((l, n, r), dtype=np.complex128)
        flags = C.c_int(0)
        src = None if x is None else _c128(x)
        self._ck(self._lib.mitdvp_heff_apply_center(self._h, None if src is None else _dp(src), _dp(out), C.byref(flags)))
        return out, flags.value

    def krylov_memory(self, isite: int) -> int:
        k = C.c_int()
        self._ck(self._lib.mitdvp_get_krylov_memory(self._h, isite, C.byref(k)))
        return k.value

    def set_small_kernels(self, on: bool):
        self._ck(self._lib.mitdvp_set_small_kernels(self._h, int(bool(on))))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        _lib.check(rc, self._h)

    # ---- host or device operands ------------------------------------------
    def _with_mode(self, mode: int, call):
        """run one library call with the pointer mode its operands need (0 host, 1 device)"""
        if mode == 0:
            return self._ck(call())
        self._ck(self._lib.mitdvp_set_pointer_mode(self._h, 1))
        try:
            return self._ck(call())
        finally:
            self._ck(self._lib.mitdvp_set_pointer_mode(self._h, 0))

    def _out(self, shape, device: bool):
        """destination of a getter: NumPy array, or a torch complex128 tensor on this engine's GPU"""
        if not device:
            a = np.empty(shape, dtype=np.complex128)
            return a, _dp(a), 0
        import torch

        t = torch.empty(tuple(shape), dtype=torch.complex128, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(t.device).synchronize()  # the allocator may hand back memory with work pending
        return t, C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_double)), 1

    # ---- state ---------------------------------------------------------
    def set_site(self, isite: int, data, gauge: str = "C"):
        a = _Operand(data)
        if a.ndim != 3:
            raise ValueError("site tensor must be (D_l, d, D_r)")
        g = {"Psi": _lib.GAUGE_PSI, "A": _lib.GAUGE_A, "B": _lib.GAUGE_B, "C": _lib.GAUGE_C}[gauge]
        self._with_mode(a.mode, lambda: self._lib.mitdvp_set_site(self._h, isite, a.ptr, a.shape[0], a.shape[1], a.shape[2], g))

    def set_mps(self, cores, canonicalize: bool = False, scale: float = 1.0):
        """cores: site-0-centred canonical MPS (gauges Psi,B,...,B), or arbitrary
        cores with ``canonicalize=True`` (alloc_superblock_random's QR sweep)."""
        for i, c in enumerate(cores):
            self.set_site(i, c, "C" if canonicalize else ("Psi" if i == 0 else "B"))
        if canonicalize:  # scale=None: keep the state's own normalisation (Liouville space)
            self._ck(self._lib.mitdvp_canonicalize(self._h, -1.0 if scale is None else scale))

    def get_site(self, isite: int, device: bool = False):
        l, n, r, g = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._ck(self._lib.mitdvp_get_site_shape(self._h, isite, C.byref(l), C.byref(n), C.byref(r), C.byref(g)))
        out, ptr, mode = self._out((l.value, n.value, r.value), device)
        self._with_mode(mode, lambda: self._lib.mitdvp_get_site(self._h, isite, ptr))
        return out

    def get_mps(self):
        return [self.get_site(i) for i in range(self.nsite)]

    def init_random(self, dims, bond_dim: int, seed: int = 1):
        arr = (C.c_int * len(dims))(*dims)
        self._ck(self._lib.mitdvp_init_random(self._h, arr, bond_dim, seed))

    def init_random_block(self, dims, first: int, bond_dim: int, seed: int = 1, balance: bool = True):
        """the raw tensors ``init_random`` draws for sites [first, first + nsite) of the chain with physical dimensions
        ``dims`` (global shapes and seeds), not canonicalised: one block of a site-sharded state (parallel_sites.py)"""
        arr = (C.c_int * len(dims))(*dims)
        self._ck(self._lib.mitdvp_init_random_block(self._h, arr, len(dims), int(first), bond_dim, seed, int(bool(balance))))

    def set_mpo(self, cores, op_id: int = 0, shift: complex = 0.0):
        cores = list(cores)
        if cores:
            self._mpo_ends = getattr(self, "_mpo_ends", {})
            self._mpo_ends[op_id] = (np.shape(cores[0])[0], np.shape(cores[-1])[-1])
            # MPO bond left / right of every site: the block a ranged fold hands back has the bond at the END of its range
            self._mpo_bonds = getattr(self, "_mpo_bonds", {})
            self._mpo_bonds[op_id] = [(np.shape(c)[0], np.shape(c)[-1]) for c in cores]
        for i, w in enumerate(cores):
            a = _c128(w)
            if a.ndim != 4:
                raise ValueError("MPO core must be (M_l, d, d, M_r)")
            self._ck(
                self._lib.mitdvp_set_mpo_core(self._h, op_id, i, _dp(a), a.shape[0], a.shape[1], a.shape[2], a.shape[3])
            )
        self._ck(self._lib.mitdvp_set_shift(self._h, op_id, complex(shift).real, complex(shift).imag))

    # ---- one block of a site-range sharded chain (include/mitdvp.h, "one block ...") ---------
    _GAUGE = {"Psi": _lib.GAUGE_PSI, "A": _lib.GAUGE_A, "B": _lib.GAUGE_B, "C": _lib.GAUGE_C}

    def replace_site(self, isite: int, data, gauge: str):
        a = _Operand(data)
        self._with_mode(a.mode, lambda: self._lib.mitdvp_replace_site(self._h, isite, a.ptr, self._GAUGE[gauge]))

    def set_boundary_env(self, side: int, block):
        a = _Operand(block)
        if a.ndim != 3 or a.shape[0] != a.shape[2]:
            raise ValueError("boundary block must be (D, M, D)")
        self._with_mode(a.mode, lambda: self._lib.mitdvp_set_boundary_env(self._h, side, a.ptr, a.shape[0], a.shape[1]))

    def get_env(self, side: int, bond: int, device: bool = False):
        d, m = C.c_int(), C.c_int()
        self._ck(self._lib.mitdvp_get_env(self._h, side, bond, None, C.byref(d), C.byref(m)))
        out, ptr, mode = self._out((d.value, m.value, d.value), device)
        self._with_mode(mode, lambda: self._lib.mitdvp_get_env(self._h, side, bond, ptr, C.byref(d), C.byref(m)))
        return out

    def build_envs(self, side: int):
        self._ck(self._lib.mitdvp_build_envs(self._h, side))

    def site_exp(self, dt_au: float):
        self._ck(self._lib.mitdvp_site_exp(self._h, dt_au))

    def split_center(self, forward: bool):
        self._ck(self._lib.mitdvp_split_center(self._h, int(forward)))

    def bond_exp(self, dt_au: float):
        self._ck(self._lib.mitdvp_bond_exp(self._h, dt_au))

    def absorb_bond(self, forward: bool):
        self._ck(self._lib.mitdvp_absorb_bond(self._h, int(forward)))

    def get_bond(self) -> np.ndarray:
        n = C.c_int()
        self._ck(self._lib.mitdvp_get_bond(self._h, None, C.byref(n)))
        out = np.empty((n.value, n.value), dtype=np.complex128)
        self._ck(self._lib.mitdvp_get_bond(self._h, _dp(out), C.byref(n)))
        return out

    def set_bond(self, bond: int, x):
        a = _c128(x)
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError("bond matrix must be square")
        self._ck(self._lib.mitdvp_set_bond(self._h, bond, _dp(a), a.shape[0]))

    def site_rdm_blocks(self, isite: int, left, right) -> np.ndarray:
        """rho[j][j'] of one site given the transfer blocks (bra, ket) of everything left / right of it."""
        a, b = _c128(left), _c128(right)
        l, n, r = self.get_site_shape(isite)[:3]
        if a.shape != (l, l) or b.shape != (r, r):
            raise ValueError("transfer blocks must be (D_l, D_l) and (D_r, D_r)")
        out = np.empty((n, n), dtype=np.complex128)
        self._ck(self._lib.mitdvp_site_rdm_blocks(self._h, isite, _dp(a), _dp(b), _dp(out)))
        return out

    def fold_block(self, block, *, op_id: int = -1, conj: bool = True, from_left: bool = True, out_shape=None, first: int = 0,
                   count: int | None = None):
        """Carry a boundary block (D, M, D) through all sites of this engine (``mitdvp_fold_block``): the piece of
        ``MPSCoefParallel.ovlp`` / ``expectation`` one rank computes.  ``op_id < 0``: plain transfer (M = 1)."""
        a = _c128(block)
        if a.ndim != 3 or a.shape[0] != a.shape[2]:
            raise ValueError("boundary block must be (D, M, D)")
        if count is None:
            count = self.nsite - first
        if count == 0:
            return a.copy()
        if out_shape is None:
            last = self.get_site_shape(first + count - 1 if from_left else first)
            dn = last[2] if from_left else last[0]
            m_out = 1
            if op_id >= 0:
                bonds = getattr(self, "_mpo_bonds", {}).get(op_id)
                if bonds is None:
                    raise ValueError("fold_block: this operator's cores were not set through set_mpo; pass out_shape")
                m_out = bonds[first + count - 1][1] if from_left else bonds[first][0]
            out_shape = (dn, m_out, dn)
        out = np.empty(out_shape, dtype=np.complex128)
        self._ck(self._lib.mitdvp_fold_block_range(self._h, op_id, int(conj), int(from_left), first, count, _dp(a), a.shape[0],
                                                   a.shape[1], _dp(out)))
        return out

    # ---- hot path ------------------------------------------------------
    def propagate(self, dt_au: float):
        self._ck(self._lib.mitdvp_step(self._h, dt_au))

    def sweep(self, dt_au: float, forward: bool):
        self._ck(self._lib.mitdvp_sweep(self._h, dt_au, int(forward)))

    def sweep_part(self, dt_au: float, forward: bool, nsites: int) -> int:
        """The next `nsites` local updates of a half-sweep (started when none is in progress) through sweep()'s own
        code; returns the sites still to go (0: the half-sweep is complete)."""
        left = C.c_int()
        self._ck(self._lib.mitdvp_sweep_part(self._h, dt_au, int(forward), int(nsites), C.byref(left)))
        return left.value

    def invalidate_env(self):
        self._ck(self._lib.mitdvp_invalidate_env(self._h))

    # ---- observables ---------------------------------------------------
    def expectation(self, op_id: int = 0) -> complex:
        out = np.zeros(2)
        self._ck(self._lib.mitdvp_expect(self._h, op_id, _dp(out)))
        return complex(out[0], out[1])

    def autocorr(self) -> complex:
        out = np.zeros(2)
        self._ck(self._lib.mitdvp_autocorr(self._h, _dp(out)))
        return complex(out[0], out[1])

    def save_reference(self) -> None:
        """Keep a device copy of the current state (the t = 0 state of a run without the t/2 trick)."""
        self._ck(self._lib.mitdvp_save_reference(self._h))

    def overlap_reference(self) -> complex:
        """<saved state | current state>."""
        out = np.zeros(2)
        self._ck(self._lib.mitdvp_overlap_reference(self._h, _dp(out)))
        return complex(out[0], out[1])

    def norm(self) -> float:
        out = C.c_double()
        self._ck(self._lib.mitdvp_norm(self._h, C.byref(out)))
        return out.value

    def site_rdm(self, isite: int) -> np.ndarray:
        d = self.get_site_shape(isite)[1]
        out = np.empty((d, d), dtype=np.complex128)
        self._ck(self._lib.mitdvp_site_rdm(self._h, isite, _dp(out)))
        return out

    def reduced_density(self, remain_nleg) -> np.ndarray:
        """``get_reduced_densities`` for one key: legs kept per site (0, 1 or 2)."""
        legs = [int(x) for x in remain_nleg]
        arr = (C.c_int * len(legs))(*legs)
        n = C.c_size_t(0)
        self._ck(self._lib.mitdvp_reduced_density(self._h, arr, len(legs), None, C.byref(n)))
        out = np.empty(n.value, dtype=np.complex128)
        self._ck(self._lib.mitdvp_reduced_density(self._h, arr, len(legs), _dp(out), C.byref(n)))
        shape = []
        for p, k in enumerate(legs):
            shape += [self.get_site_shape(p)[1]] * k
        return out.reshape(shape)

    def operate(self, op_id: int = 0, maxstep: int = 10, conv_tol: float = 1.0e-8):
        """``Simulator.operate``: replace the state by O|psi> / ||O|psi>|| fitted in the current
        bond dimensions; returns (norm of the last apply, double sweeps done)."""
        nrm, it = C.c_double(), C.c_int()
        self._ck(self._lib.mitdvp_operate(self._h, op_id, maxstep, conv_tol, C.byref(nrm), C.byref(it)))
        return nrm.value, it.value

    def set_gates(self, gates: dict | None) -> None:
        """Register one-site gates ``{site: U}`` (``Model(one_gate_to_apply=...)``): U is
        d x d (U[d_out, d_in]) or a length-d diagonal; ``propagate`` applies them between its
        half-sweeps.  ``None`` / ``{}`` removes all gates."""
        for i in range(self.nsite):
            self._ck(self._lib.mitdvp_set_gate(self._h, i, None, 0))
        self._step_gates = dict(gates or {})
        for site, U in (gates or {}).items():
            U = np.asarray(U, dtype=np.complex128)
            if U.ndim == 1:
                U = np.diag(U)
            if U.ndim != 2 or U.shape[0] != U.shape[1]:
                raise ValueError("a gate must be a square matrix or a diagonal")
            U = np.ascontiguousarray(U)
            self._ck(self._lib.mitdvp_set_gate(self._h, int(site), _dp(U), U.shape[0]))

    def apply_gates(self) -> None:
        """``apply_one_gate`` now, re-orthogonalising towards the current centre site."""
        self._ck(self._lib.mitdvp_apply_gates(self._h))

    def set_kraus(self, kraus: dict | None) -> None:
        """Register Kraus maps ``{(site,): B}`` / ``{(site, site + 1): B}`` with B of shape
        (k, d, d) (``Model(kraus_op=...)``); ``propagate`` applies them after the gates,
        between its half-sweeps.  ``None`` / ``{}`` removes all maps."""
        for i in range(self.nsite):
            self._ck(self._lib.mitdvp_set_kraus(self._h, i, 0, None, 0, 0))
        for sites, B in (kraus or {}).items():
            sites = tuple(int(x) for x in (sites if isinstance(sites, (tuple, list)) else (sites,)))
            B = np.ascontiguousarray(np.asarray(B, dtype=np.complex128))
            if B.ndim != 3 or B.shape[1] != B.shape[2]:
                raise ValueError("a Kraus tensor must have shape (k, d, d)")
            if len(sites) == 2 and sites[0] + 1 != sites[1]:
                raise ValueError(f"site_inds={sites} is not nearest neighbour")
            if len(sites) not in (1, 2):
                raise ValueError(f"site_inds={sites} is not yet implemented")
            self._ck(self._lib.mitdvp_set_kraus(self._h, sites[0], int(len(sites) == 2), _dp(B), B.shape[0], B.shape[1]))

    def apply_kraus(self) -> None:
        """``apply_kraus`` now, re-orthogonalising towards the current centre site."""
        self._ck(self._lib.mitdvp_apply_kraus(self._h))

    def set_adaptive(self, enable: bool = True, Dmax: int = 20, dD: int = 5, p_proj: float = 1.0e-4) -> None:
        """Adaptive bond dimension (``Simulator.propagate(adaptive=True, adaptive_Dmax=...,
        adaptive_dD=..., adaptive_p_proj=...)``): ranks grow by up to ``dD`` per half-sweep
        where the projection error asks for it, never above ``Dmax``."""
        self._ck(self._lib.mitdvp_set_adaptive(self._h, int(bool(enable)), int(Dmax), int(dD), float(p_proj)))

    def bond_dims(self) -> list[int]:
        """Current bond dimensions (``WFunc.bonddim``)."""
        return [self.get_site_shape(i)[2] for i in range(self.nsite - 1)]

    def truncate_bond(self, p: float, max_dim: int = 0):
        """SVD-truncate the bond right of the centre site (``truncate_sigvec``).
        Returns (new bond dimension, kept singular values normalised to unit norm)."""
        l, n, r, g = self.get_site_shape(self._center())
        sv = np.zeros(r)
        nd = C.c_int()
        self._ck(self._lib.mitdvp_truncate_bond(self._h, p, max_dim, C.byref(nd), _dp(sv)))
        return nd.value, sv[: nd.value].copy()

    def _center(self) -> int:
        for i in range(self.nsite):
            if self.get_site_shape(i)[3] == _lib.GAUGE_PSI:
                return i
        raise ValueError("no centre site")

    # ---- Liouville space (vectorised density matrices) -------------------
    def set_trace_op(self, cores, op_id: int):
        """Full-chain observable with n-dimensional physical legs (site dim = n*n)."""
        for i, w in enumerate(cores):
            a = _c128(w)
            if a.ndim != 4 or a.shape[1] != a.shape[2]:
                raise ValueError("trace operator core must be (M_l, n, n, M_r)")
            self._ck(self._lib.mitdvp_set_trace_op_core(self._h, op_id, i, _dp(a), a.shape[0], a.shape[1], a.shape[3]))

    def set_subspace(self, isite: int, n: int, inds):
        """Subspace projection of a Liouville-space site (``Model(subspace_inds=...)``, _mps_mpo.py:135-220): the
        physical leg of ``isite`` holds the entries ``inds`` of the n*n vectorised density matrix.  Before
        ``set_trace_op`` for that site; the sweep itself only sees the shorter leg."""
        inds = [int(x) for x in inds]
        arr = (C.c_int * max(1, len(inds)))(*inds)
        self._ck(self._lib.mitdvp_set_subspace(self._h, int(isite), int(n), arr, len(inds)))
        self._sub_n = dict(getattr(self, "_sub_n", {}))
        if inds:
            self._sub_n[int(isite)] = int(n)
        else:
            self._sub_n.pop(int(isite), None)

    def hermitise(self):
        """``MPSCoef.hermitise`` (_mps_cls.py:2289-2312): rho <- (rho + rho^dagger) / 2, bonds re-truncated to their
        old dimensions, site-0-centred canonical form."""
        self._ck(self._lib.mitdvp_hermitise(self._h))

    def expect_trace(self, op_id: int) -> complex:
        out = np.zeros(2)
        self._ck(self._lib.mitdvp_expect_trace(self._h, op_id, _dp(out)))
        return complex(out[0], out[1])

    def partial_trace(self, remain_nleg) -> np.ndarray:
        legs = [int(x) for x in remain_nleg]
        arr = (C.c_int * len(legs))(*legs)
        n = C.c_size_t(0)
        self._ck(self._lib.mitdvp_partial_trace(self._h, arr, len(legs), None, C.byref(n)))
        out = np.empty(n.value, dtype=np.complex128)
        self._ck(self._lib.mitdvp_partial_trace(self._h, arr, len(legs), _dp(out), C.byref(n)))
        center = max(i for i, k in enumerate(legs) if k)
        shape = []
        for p in range(center + 1):
            nn = getattr(self, "_sub_n", {}).get(p) or int(round(self.get_site_shape(p)[1] ** 0.5))
            shape += [nn] * (2 if p == center else legs[p])
        return out.reshape(shape)

    def get_site_shape(self, isite: int):
        l, n, r, g = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._ck(self._lib.mitdvp_get_site_shape(self._h, isite, C.byref(l), C.byref(n), C.byref(r), C.byref(g)))
        return l.value, n.value, r.value, g.value

    def krylov_stats(self):
        arr = (C.c_int * self.nsite)()
        self._ck(self._lib.mitdvp_krylov_stats(self._h, arr))
        return list(arr)

    def counters(self) -> dict:
        c = _lib.Counters()
        self._ck(self._lib.mitdvp_counters_get(self._h, C.byref(c)))
        return c.as_dict()

    def counters_reset(self):
        self._ck(self._lib.mitdvp_counters_reset(self._h))

    def set_profiling(self, on: bool):
        self._ck(self._lib.mitdvp_set_profiling(self._h, int(on)))


class MultiStateEngine(TDVPEngine):
    """Several electronic states (MPS-SM, ``nstate > 1``): one MPS per state, one MPO block and
    one scalar ``coupleJ`` per (bra, ket) state pair; the local solves act on the states' centre
    tensors stacked into one vector (reference: ``superblock_states[istate][isite]``,
    ``TensorHamiltonian.mpo[i][j]``, ``multiplyH_MPS_direct_MPO.dot``)."""

    def __init__(self, nsite: int, nstate: int, **kw):
        super().__init__(nsite, **kw)
        self.nstate = nstate
        self._ck(self._lib.mitdvp_ms_configure(self._h, nstate))

    def set_state(self, istate: int, cores, canonicalize: bool = False, scale: float = 1.0):
        """Site-0-centred cores of one state (gauges Psi,B,...,B), or arbitrary cores with
        ``canonicalize=True`` once ALL states are set (``canonicalize_states``)."""
        for p, c in enumerate(cores):
            a = _c128(c)
            if a.ndim != 3:
                raise ValueError("site tensor must be (D_l, d, D_r)")
            g = _lib.GAUGE_C if canonicalize else (_lib.GAUGE_PSI if p == 0 else _lib.GAUGE_B)
            self._ck(self._lib.mitdvp_ms_set_site(self._h, istate, p, _dp(a), a.shape[0], a.shape[1], a.shape[2], g))

    def set_states(self, states, weights=None):
        """states[istate] = arbitrary cores; QR sweep per state and site 0 scaled to
        sqrt(weight / sum(weights)) (alloc_superblock_random with init_weight_ESTATE)."""
        if len(states) != self.nstate:
            raise ValueError("one list of cores per state")
        for s, cores in enumerate(states):
            self.set_state(s, cores, canonicalize=weights is not None)
        if weights is not None:
            w = np.asarray(weights, dtype=float)
            if len(w) != self.nstate or w.min() < 0 or w.sum() <= 0:
                raise ValueError("weights must be non-negative, one per state")
            w = w / w.sum()
            for s in range(self.nstate):
                self._ck(self._lib.mitdvp_ms_canonicalize(self._h, s, float(np.sqrt(w[s]))))

    def get_state_site(self, istate: int, isite: int) -> np.ndarray:
        l, n, r, g = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._ck(self._lib.mitdvp_ms_get_site_shape(self._h, istate, isite, C.byref(l), C.byref(n), C.byref(r), C.byref(g)))
        out = np.empty((l.value, n.value, r.value), dtype=np.complex128)
        self._ck(self._lib.mitdvp_ms_get_site(self._h, istate, isite, _dp(out)))
        return out

    def get_states(self):
        return [[self.get_state_site(s, p) for p in range(self.nsite)] for s in range(self.nstate)]

    def set_block(self, ibra: int, iket: int, cores, op_id: int = 0):
        for p, w in enumerate(cores):
            a = _c128(w)
            if a.ndim != 4:
                raise ValueError("MPO core must be (M_l, d, d, M_r)")
            self._ck(self._lib.mitdvp_ms_set_mpo_core(self._h, op_id, ibra, iket, p, _dp(a), *a.shape))

    def set_hamiltonian(self, blocks, coupleJ=None, op_id: int = 0):
        """blocks[i][j] = full-chain MPO cores or None; coupleJ[i][j] scalars."""
        for i in range(self.nstate):
            for j in range(self.nstate):
                if blocks[i][j] is not None:
                    self.set_block(i, j, blocks[i][j], op_id)
                c = 0.0 if coupleJ is None else complex(coupleJ[i][j])
                self._ck(self._lib.mitdvp_ms_set_coupleJ(self._h, op_id, i, j, complex(c).real, complex(c).imag))

    def propagate(self, dt_au: float):
        self._ck(self._lib.mitdvp_ms_step(self._h, dt_au))

    def expectation(self, op_id: int = 0) -> complex:
        out = np.zeros(2)
        self._ck(self._lib.mitdvp_ms_expect(self._h, op_id, _dp(out)))
        return complex(out[0], out[1])

    def autocorr(self) -> complex:
        out = np.zeros(2)
        self._ck(self._lib.mitdvp_ms_autocorr(self._h, _dp(out)))
        return complex(out[0], out[1])

    def operate(self, op_id: int = 0, maxstep: int = 10, conv_tol: float = 1.0e-8):
        nrm, it = C.c_double(), C.c_int()
        self._ck(self._lib.mitdvp_ms_operate(self._h, op_id, maxstep, conv_tol, C.byref(nrm), C.byref(it)))
        return nrm.value, it.value

    def pop_states(self) -> list[float]:
        out = np.zeros(self.nstate)
        self._ck(self._lib.mitdvp_ms_pops(self._h, _dp(out)))
        return [float(x) for x in out]

    def norm(self) -> float:
        return float(np.sqrt(sum(self.pop_states())))


# ---- unit-level seam (SURVEY 8b "internal seam 1") ---------------------------
def heff_apply(L, W, R, psi, device=0, reps=0):
    L, W, R, psi = map(_c128, (L, W, R, psi))
    dl, d, dr = psi.shape
    out = np.empty_like(psi)
    ms = C.c_double()
    _lib.check(
        _lib.load().mitdvp_heff_apply(
            device, _dp(L), _dp(W), _dp(R), _dp(psi), dl, d, dr, W.shape[0], W.shape[3], _dp(out), reps, C.byref(ms)
        )
    )
    return (out, ms.value) if reps else out


def keff_apply(L, R, sval, device=0):
    L, R, sval = map(_c128, (L, R, sval))
    out = np.empty_like(sval)
    _lib.check(_lib.load().mitdvp_keff_apply(device, _dp(L), _dp(R), _dp(sval), sval.shape[0], sval.shape[1], L.shape[1], _dp(out)))
    return out


def env_update(env, site, W, left: bool, device=0):
    env, site, W = map(_c128, (env, site, W))
    dl, d, dr = site.shape
    ml, mr = W.shape[0], W.shape[3]
    out = np.empty((dr, mr, dr) if left else (dl, ml, dl), dtype=np.complex128)
    _lib.check(_lib.load().mitdvp_env_update(device, int(left), _dp(env), _dp(site), _dp(W), dl, d, dr, ml, mr, _dp(out)))
    return out


_SMALL_KINDS = {"heff": _lib.SMALL_HEFF, "keff": _lib.SMALL_KEFF, "env": _lib.SMALL_ENV}


def small_plan(kind: str, dims, exp_mode: bool = False, n_cu: int = 256):
    """The launch plan of the one-launch small-bond kernel for a chain on ``n_cu`` compute units (host arithmetic, no GPU):
    ``kind`` "heff" with dims (dl, d, dr, ml, mr), "keff" (d1, d2, m) or "env" (din, min, d, dout, mout).  A dict with
    ok, nsc, cs, spw, a_resident, grid, lds_bytes, sg_aliases_x; ok = 0 where the chain does not qualify."""
    q = (C.c_int * len(dims))(*[int(x) for x in dims])
    if len(dims) != (3 if kind == "keff" else 5):
        raise ValueError(f"{kind}: {len(dims)} dims")
    out = _lib.SmallPlan()
    _lib.check(_lib.load().mitdvp_small_plan(_SMALL_KINDS[kind], q, int(bool(exp_mode)), int(n_cu), C.byref(out)))
    return out.as_dict()


def small_apply(kind: str, operands, shift=0.0, cu_count: int = 0, left: bool = True, device=0):
    """One H_eff / K_eff apply or environment update through the engine's production dispatch, on an engine confined to
    the compute units [0, cu_count) (0: the whole device), with a complex ``shift`` (H_eff, K_eff).  ``operands``:
    "heff" (L, W, R, psi), "keff" (L, R, sigma), "env" (env, site, W) with ``left``.  Returns (out, info): info["n_launch"]
    is 1 when the one-launch kernel served the call, and info["plan"] is then the plan it ran."""
    ops = [_c128(x) for x in operands]
    null = C.POINTER(C.c_double)()
    if kind == "heff":
        L, W, R, v = ops
        dims = (*v.shape, W.shape[0], W.shape[3])
        a, w, r, out = L, W, R, np.empty_like(v)
    elif kind == "keff":
        L, R, v = ops
        dims = (v.shape[0], v.shape[1], L.shape[1])
        a, w, r, out = L, None, R, np.empty_like(v)
    else:
        a, v, w = ops
        dl, d, dr = v.shape
        ml, mr = w.shape[0], w.shape[3]
        dims, r = (dl, d, dr, ml, mr), None
        out = np.empty((dr, mr, dr) if left else (dl, ml, dl), dtype=np.complex128)
    q = (C.c_int * len(dims))(*dims)
    info = _lib.SmallInfo()
    s = complex(shift)
    _lib.check(_lib.load().mitdvp_small_apply(
        device, int(cu_count), _SMALL_KINDS[kind], int(bool(left)), q, _dp(a), null if w is None else _dp(w),
        null if r is None else _dp(r), _dp(v), s.real, s.imag, _dp(out), C.byref(info)))
    return out, {"n_launch": info.n_launch, "plan": info.plan.as_dict()}


def gauge_trf(psi, key: str, device=0):
    """key: "Psi2Asigma" -> (A, sigma);  "Psi2sigmaB" -> (B, sigma)."""
    psi = _c128(psi)
    dl, d, dr = psi.shape
    k = {"Psi2Asigma": 0, "Psi2sigmaB": 1}[key]
    site = np.empty_like(psi)
    sig = np.empty((dr, dr) if k == 0 else (dl, dl), dtype=np.complex128)
    _lib.check(_lib.load().mitdvp_gauge_trf(device, k, _dp(psi), dl, d, dr, _dp(site), _dp(sig)))
    return site, sig


def expm_dense(mat, x, scale, integrator="lanczos", conserve_norm=True, thresh=1e-9, k_prev=0, variant="reference", device=0,
               counters=False):
    """``counters=True``: also the counters of the engine that ran the solve (``n_launch`` without the operator's GEMM)"""
    mat, xx = _c128(mat), _c128(x)
    y = np.empty_like(xx)
    k = C.c_int()
    cnt = _lib.Counters()
    s = complex(scale)
    _lib.check(
        _lib.load().mitdvp_expm_dense_counted(
            device,
            {"lanczos": 0, "arnoldi": 1}[integrator],
            int(conserve_norm),
            {"reference": 0, "orthodox": 1}[variant],
            _dp(mat),
            mat.shape[0],
            _dp(xx),
            s.real,
            s.imag,
            thresh,
            k_prev,
            _dp(y),
            C.byref(k),
            C.byref(cnt),
        )
    )
    return (y, k.value, cnt.as_dict()) if counters else (y, k.value)


def zgemm(A, B, C0=None, transA=False, conjA=False, transB=False, conjB=False, alpha=1.0, beta=0.0, tile_cfg=-1, reps=0, device=0):
    """C = alpha*op(A)*op(B) + beta*C0 on the MFMA kernel (row-major)."""
    A, B = _c128(A), _c128(B)
    m, k = (A.shape[1], A.shape[0]) if transA else A.shape
    n = B.shape[0] if transB else B.shape[1]
    Cm = np.zeros((m, n), dtype=np.complex128) if C0 is None else _c128(C0).copy()
    al = np.array([complex(alpha).real, complex(alpha).imag])
    be = np.array([complex(beta).real, complex(beta).imag])
    ms = C.c_double()
    _lib.check(
        _lib.load().mitdvp_zgemm(
            device, int(transA), int(conjA), int(transB), int(conjB), m, n, k, _dp(A), _dp(B), _dp(Cm), _dp(al), _dp(be), tile_cfg, reps, C.byref(ms)
        )
    )
    return (Cm, ms.value) if reps else Cm


ZGEMM_DESC_DEFAULTS = dict(
    m=0, n=0, k=0, batch=1, transA=0, conjA=0, transB=0, conjB=0, lda=0, ldb=0, ldc=0, strideA=0, strideB=0, strideC=0,
    offA=0, offB=0, offC=0, alpha=1.0, beta=0.0, tile_cfg=-1, mode3m=-1, arow_skip=0, rowmap_p=0, rowmap_s1=0, rowmap_s2=0,
    rowmap_r0=0, klist_stride=0)


def zgemm_desc(args: dict, A, B, Cbuf, klist=None, device=0) -> np.ndarray:
    """One product of the MFMA kernel through its whole descriptor (``mitdvp_zgemm_desc``): ``args`` holds the fields of
    ``mitdvp_zgemm_args`` (missing ones as in ``ZGEMM_DESC_DEFAULTS``), ``A``, ``B``, ``Cbuf`` are whole flat buffers
    that the views of the descriptor lie in.  Returns the whole C buffer after the product; ``Cbuf`` is not modified.
    A descriptor that leaves a buffer, or that the kernel does not serve, raises ValueError before the GPU is touched."""
    unknown = set(args) - set(ZGEMM_DESC_DEFAULTS)
    if unknown:
        raise TypeError(f"zgemm_desc: unknown descriptor fields {sorted(unknown)}")
    v = dict(ZGEMM_DESC_DEFAULTS, **args)
    a = _lib.ZgemmArgs()
    for name, val in v.items():
        if name in ("alpha", "beta"):
            z = complex(val)
            setattr(a, name, (C.c_double * 2)(z.real, z.imag))
        else:
            setattr(a, name, int(val))
    A, B = _c128(A).reshape(-1), _c128(B).reshape(-1)
    out = _c128(Cbuf).reshape(-1).copy()
    kl = None if klist is None else np.ascontiguousarray(klist, dtype=np.intc).reshape(-1)
    _lib.check(
        _lib.load().mitdvp_zgemm_desc(
            device, C.byref(a), _dp(A), A.size, _dp(B), B.size, _dp(out), out.size,
            None if kl is None else kl.ctypes.data_as(C.POINTER(C.c_int)), 0 if kl is None else kl.size,
        )
    )
    return out


ZGEMM_REDUCE_DEFAULTS = dict(
    m=0, n=0, k=0, transB=0, lda=0, ldb=0, offA=0, offB=0, xm=0, yn=0, di=0, acc=0, ldw=0, offW=0, su=0, sv=0, si=0, offC=0,
    mode3m=-1, epi_b4=-1, epi_full=-1)


def zgemm_reduce(args: dict, A, B, W, Cbuf, device=0):
    """One product of the MFMA kernel with its reducing epilogue (``mitdvp_zgemm_reduce``), as a side of the edge form of
    an H_eff apply issues it: ``args`` holds the fields of ``mitdvp_zgemm_reduce_args`` (missing ones as in
    ``ZGEMM_REDUCE_DEFAULTS``); ``A``, ``B``, ``W``, ``Cbuf`` are whole flat buffers.  Returns ``(C_out, variant)``: the whole
    C buffer after the product (``Cbuf`` is not modified) and the number, 1..13, of the epilogue body that ran.  A
    descriptor that leaves a buffer, or that the kernel does not serve, raises ValueError before the GPU is touched."""
    unknown = set(args) - set(ZGEMM_REDUCE_DEFAULTS)
    if unknown:
        raise TypeError(f"zgemm_reduce: unknown descriptor fields {sorted(unknown)}")
    a = _lib.ZgemmReduceArgs()
    for name, val in dict(ZGEMM_REDUCE_DEFAULTS, **args).items():
        setattr(a, name, int(val))
    A, B, W = _c128(A).reshape(-1), _c128(B).reshape(-1), _c128(W).reshape(-1)
    out = _c128(Cbuf).reshape(-1).copy()
    variant = C.c_int(0)
    _lib.check(
        _lib.load().mitdvp_zgemm_reduce(
            device, C.byref(a), _dp(A), A.size, _dp(B), B.size, _dp(W), W.size, _dp(out), out.size, C.byref(variant)
        )
    )
    return out, variant.value


BATCH_BLOCK_OPS = {"matmul": _lib.BLOCK_MATMUL, "heff": _lib.BLOCK_HEFF, "keff": _lib.BLOCK_KEFF, "env": _lib.BLOCK_ENV,
                   "overlap": _lib.BLOCK_OVERLAP, "qr": _lib.BLOCK_QR, "split": _lib.BLOCK_SPLIT}


def pack_w2(core, order: str) -> np.ndarray:
    """The matrix a batch kernel reads an MPO core ``W[c, i, j, t]`` of shape (ml, d, d, mr) as (``MpoSite`` in
    csrc/engine.h): ``w2l[(i,t)][(c,j)]`` (the W stage of H_eff), ``w2el[(t,j)][(i,c)]`` (environment update ->),
    ``w2er[(c,j)][(i,t)]`` (environment update <-)."""
    W = _c128(core)
    ml, d, d2, mr = W.shape
    if d != d2:
        raise ValueError("pack_w2: need a square 4-leg core")
    if order == "w2l":
        return np.ascontiguousarray(W.transpose(1, 3, 0, 2)).reshape(d * mr, ml * d)
    if order == "w2el":
        return np.ascontiguousarray(W.transpose(3, 2, 1, 0)).reshape(mr * d, d * ml)
    if order == "w2er":
        return np.ascontiguousarray(W.transpose(0, 2, 1, 3)).reshape(ml * d, d * mr)
    raise ValueError(f"pack_w2: unknown order {order!r}")


def batch_block_footprint(op: str, dims) -> dict:
    """Elements per copy of the results of ``batch_block``: ``out0`` and ``out1`` complex, ``info`` doubles (the table in
    csrc/batch_block_check.h, which is what decides)."""
    q = [int(v) for v in dims]
    if op == "matmul":
        return dict(out0=q[0] * q[1], out1=0, info=1)
    if op == "heff":
        return dict(out0=q[0] * q[1] * q[2], out1=0, info=1)
    if op == "keff":
        return dict(out0=q[0] * q[0], out1=0, info=1)
    if op == "env":
        return dict(out0=q[3] * q[4] * q[3], out1=0, info=1)
    if op == "overlap":
        return dict(out0=1, out1=0, info=1)
    if op == "qr":
        return dict(out0=q[0] * q[1], out1=q[1] * q[1], info=1)
    if op == "split":
        return dict(out0=q[2] * q[1], out1=q[0] * q[2], info=3 + q[0])
    raise ValueError(f"batch_block: unknown op {op!r}")


def batch_block(op: str, dims, *operands, ncopies=1, variant=0, scl=1.0, device=0):
    """One building block of the batched-trajectory kernels in one workgroup per copy (``mitdvp_batch_block``; include/mitdvp.h
    has the operations, their dims, variants and operand order).  ``operands``: up to four arrays in the layouts the kernels
    see (``pack_w2`` for an MPO core), ``None`` for one the operation does not take.  Returns ``(out0, out1, info)`` with a
    leading axis of ``ncopies``.  What lies outside the kernels' envelope raises ValueError before the GPU is touched."""
    if op not in BATCH_BLOCK_OPS:
        raise ValueError(f"batch_block: unknown op {op!r}")
    if len(operands) > 4 or len(dims) > 8:
        raise TypeError("batch_block: at most four operands and eight dims")
    a = _lib.BatchBlockArgs()
    a.op, a.variant, a.ncopies, a.scl = BATCH_BLOCK_OPS[op], int(variant), int(ncopies), float(scl)
    for k, v in enumerate(dims):
        a.dims[k] = int(v)
    ins = [None if x is None else _c128(x).reshape(-1) for x in operands] + [None] * (4 - len(operands))
    nc = max(int(ncopies), 0)
    try:
        foot = batch_block_footprint(op, list(dims) + [0] * 8)
    except (OverflowError, MemoryError):
        foot = dict(out0=0, out1=0, info=1)
    if nc > 16 or min([int(v) for v in dims] or [0]) < 1 or max(foot.values()) > 1 << 24:
        foot = dict(out0=0, out1=0, info=1)  # refused below by the library, which is what decides: nothing to allocate
    out0 = np.zeros((nc, foot["out0"]), np.complex128)
    out1 = np.zeros((nc, foot["out1"]), np.complex128)
    info = np.zeros((nc, foot["info"]))
    args = []
    for x in ins:
        args += [None, 0] if x is None else [_dp(x), x.size]
    _lib.check(_lib.load().mitdvp_batch_block(device, C.byref(a), *args, _dp(out0), out0.size, _dp(out1), out1.size, _dp(info), info.size))
    return out0, out1, info


VECOP_OPS = {name: k for k, name in enumerate(_lib.VECOP_NAMES)}


def tridiag_lowest(alpha, beta, device=0):
    """The lowest eigenpair of real symmetric tridiagonal matrices of order 1 .. 64 by the device function that
    ``k_batch_relax`` runs after every Lanczos vector (``mitdvp_batch_trilow``, one workgroup per matrix).  ``alpha`` /
    ``beta``: the diagonal (k numbers) and the off-diagonal (k - 1) of one matrix, or lists of them.  Returns
    ``(theta, vec)`` -- the eigenvalue and its unit eigenvector, first component non-negative -- or two lists."""
    single = np.ndim(alpha[0]) == 0 if len(alpha) else True
    al = [alpha] if single else list(alpha)
    be = [beta] if single else list(beta)
    if len(al) != len(be) or not al:
        raise ValueError("tridiag_lowest: one off-diagonal per diagonal, at least one matrix")
    n = len(al)
    A = np.zeros((n, 64), dtype=np.float64)
    Bm = np.zeros((n, 64), dtype=np.float64)
    ks = np.zeros(n, dtype=np.int32)
    for q, (a, b) in enumerate(zip(al, be)):
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        b = np.asarray(b, dtype=np.float64).reshape(-1)
        if b.size != max(a.size - 1, 0):
            raise ValueError(f"tridiag_lowest: matrix {q} has {a.size} diagonal and {b.size} off-diagonal entries")
        ks[q] = a.size  # an order outside 1 .. 64 is the library's to refuse
        A[q, :min(a.size, 64)] = a[:64]
        Bm[q, :min(b.size, 64)] = b[:64]
    theta = np.zeros(n, dtype=np.float64)
    vec = np.zeros((n, 64), dtype=np.float64)
    lib = _lib.load()
    _lib.check(lib.mitdvp_batch_trilow(int(device), _dp(A), _dp(Bm), ks.ctypes.data_as(C.POINTER(C.c_int)), n, _dp(theta), _dp(vec)))
    vecs = [vec[q, :ks[q]].copy() for q in range(n)]
    return (float(theta[0]), vecs[0]) if single else (list(theta), vecs)


def vecop(op: str, dims, strides=(), *, variant=0, z=(), r=None, idx=None, mask=(1 << 64) - 1, zo=(), ro=None, a=1.0, b=0.0,
          both=0.0, eps=0.0, coef=(), f=(), device=0):
    """One call of one host wrapper of csrc/vecops.h on a stream of its own (``mitdvp_vecop``; include/mitdvp.h has the ops,
    their dims, strides, variants and buffers).  ``z``: up to three complex inputs, ``r`` a real input, ``idx`` an int array,
    ``zo``: up to two complex results and ``ro`` a real result, all flat and whole; ``None`` for a buffer the op does not
    take.  The results are in-out: returns ``(zo0, zo1, ro)``, copies of the caller's buffers as the device left them
    (``None`` where none was given).  A descriptor that leaves a buffer raises ValueError before the GPU is touched."""
    if op not in VECOP_OPS:
        raise ValueError(f"vecop: unknown op {op!r}")
    if len(dims) > 5 or len(strides) > 5 or len(z) > 3 or len(zo) > 2 or len(coef) > 21 or len(f) > 64:
        raise TypeError("vecop: at most five dims and strides, three inputs, two results, 21 coefficients and 64 factors")
    g = _lib.VecopArgs()
    g.op, g.variant, g.eps = VECOP_OPS[op], int(variant), float(eps)
    for k, v in enumerate(dims):
        g.dims[k] = int(v)
    for k, v in enumerate(strides):
        g.strides[k] = int(v)
    for name, val in (("a", a), ("b", b), ("both", both)):
        getattr(g, name)[0], getattr(g, name)[1] = complex(val).real, complex(val).imag
    for k, v in enumerate(coef):
        g.coef[2 * k], g.coef[2 * k + 1] = complex(v).real, complex(v).imag
    for k, v in enumerate(f):
        g.f[2 * k], g.f[2 * k + 1] = complex(v).real, complex(v).imag
    zin = [None if x is None else _c128(x).reshape(-1) for x in z] + [None] * (3 - len(z))
    zout = [None if x is None else _c128(x).reshape(-1).copy() for x in zo] + [None] * (2 - len(zo))
    rin = None if r is None else np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    rout = None if ro is None else np.array(ro, dtype=np.float64).reshape(-1)
    ind = None if idx is None else np.ascontiguousarray(idx, dtype=np.intc).reshape(-1)
    args = []
    for x in zin:
        args += [None, 0] if x is None else [_dp(x), x.size]
    args += [None, 0] if rin is None else [_dp(rin), rin.size]
    args += [None, 0] if ind is None else [ind.ctypes.data_as(C.POINTER(C.c_int)), ind.size]
    args.append(int(mask) & ((1 << 64) - 1))
    for x in zout:
        args += [None, 0] if x is None else [_dp(x), x.size]
    args += [None, 0] if rout is None else [_dp(rout), rout.size]
    _lib.check(_lib.load().mitdvp_vecop(device, C.byref(g), *args))
    return zout[0], zout[1], rout


def thin_to_full(site, gauge: str, delta_rank: int, device=0) -> np.ndarray:
    """``SiteCoef.thin_to_full``: widen an "A" (or "B") isometry by ``delta_rank``
    orthonormal columns (rows) of its orthogonal complement (capped at its dimension)."""
    site = _c128(site)
    l, c, r = site.shape
    if gauge not in ("A", "B"):
        raise ValueError(f"Invalid gauge: {gauge}")
    extra = min(int(delta_rank), l * c - r if gauge == "A" else c * r - l)
    out = np.empty((l, c, r + extra) if gauge == "A" else (l + extra, c, r), np.complex128)
    _lib.check(_lib.load().mitdvp_thin_to_full(device, 0 if gauge == "A" else 1, _dp(site), l, c, r, extra, _dp(out)))
    return out


def clock_probe(iters: int = 200000, device=0) -> dict:
    """Shader clock seen by a short single-wavefront kernel (MHz) and its duration (us)."""
    out = np.zeros(2)
    _lib.check(_lib.load().mitdvp_clock_probe(device, int(iters), _dp(out)))
    return {"mhz": 100.0 * out[0] / max(out[1], 1.0), "us": out[1] / 100.0, "cycles_per_iter": out[0] / iters}


def svd(A, device=0):
    """A = U diag(S) Vh with the engine's one-sided Jacobi kernel; returns (U, S, Vh, sweeps)."""
    A = _c128(A)
    r, c = A.shape
    k = min(r, c)
    U, S, Vh = np.empty((r, k), np.complex128), np.empty(k), np.empty((k, c), np.complex128)
    sw = C.c_int()
    _lib.check(_lib.load().mitdvp_svd(device, _dp(A), r, c, _dp(U), _dp(S), _dp(Vh), C.byref(sw)))
    return U, S, Vh, sw.value


def heff_selfcheck(dl, d, dr, ml, mr, device=0) -> dict:
    """Size-independent checks of one H_eff apply on device-resident operands."""
    out = np.zeros(4)
    _lib.check(_lib.load().mitdvp_heff_selfcheck(device, dl, d, dr, ml, mr, _dp(out)))
    return {"rel_3m_vs_4m": out[0], "linearity_defect": out[1], "norm_Hx": out[2], "ms": out[3]}


class TDVPEnsemble:
    """B independent trajectories (replicas) of one model on ONE GPU, each on its own slice of the chip.

    The small-bond regime (C2) is latency bound: one trajectory's one-launch local exponentials keep 32-128
    of the 256 compute units busy for tens of microseconds at a time.  Here every replica is an engine whose stream is
    confined to ``n_cu / B`` compute units of its own (``mitdvp_config.cu_first / cu_count``), so the replicas' launches
    overlap without admission control, and ``propagate`` is ONE library call (``mitdvp_ensemble_step``: a host thread
    per replica inside the library).  The reference runs trajectories one after the other in a Python loop
    (tests/test_mixedstate.py:269-308).  Results are those of the same engines stepped one at a time, bit for bit.
    """

    def __init__(self, n_replicas: int, nsite: int, *, device: int = 0, n_cu: int | None = None, **engine_kw):
        if n_replicas < 1:
            raise ValueError("n_replicas must be >= 1")
        if n_cu is None:
            n_cu = device_cu_count(device)
        per = (n_cu // n_replicas) // 8 * 8
        if per < 8:
            raise ValueError(f"{n_replicas} replicas do not fit {n_cu} compute units (8 per replica at least)")
        self.cu_per_replica = per
        self.engines = []
        try:
            for r in range(n_replicas):
                self.engines.append(TDVPEngine(nsite, device=device, cu_range=(r * per, per), **engine_kw))
        except Exception:
            self.close()
            raise
        self._lib = _lib.load()

    def __len__(self):
        return len(self.engines)

    def __getitem__(self, i):
        return self.engines[i]

    def set_mpo(self, cores, op_id: int = 0):
        for e in self.engines:
            e.set_mpo(cores, op_id)

    def propagate(self, dt_au: float, nsteps: int = 1):
        """``nsteps`` time steps of every replica, all replicas at once."""
        n = len(self.engines)
        hs = (C.c_void_p * n)(*[e._h for e in self.engines])
        st = (C.c_int * n)()
        rc = self._lib.mitdvp_ensemble_step(hs, n, float(dt_au), int(nsteps), st)
        if rc != 0:
            bad = next(i for i in range(n) if st[i] != 0)
            _lib.check(st[bad], self.engines[bad]._h)

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []


def density_key_legs(key, nsite: int) -> list[int]:
    """A reduced-density key in the reference's form -- a tuple of site indices, non-decreasing, each site once (its
    diagonal) or twice (ket and bra leg) -- as the legs kept per site of an ``nsite`` chain: ``(0, 0, 2, 2)`` ->
    ``[2, 0, 2]``, ``(0, 1)`` -> ``[1, 1]``.  ``ValueError`` naming the key otherwise.  Pure Python."""
    try:
        k = tuple(int(s) for s in key)
    except TypeError:
        raise ValueError(f"reduced-density key {key!r}: a key is a tuple of site indices") from None
    if not k:
        raise ValueError(f"reduced-density key {k}: it names no site")
    if any(not 0 <= s < nsite for s in k):
        raise ValueError(f"reduced-density key {k}: site out of range (the chain has {nsite} sites)")
    if any(b < a for a, b in zip(k, k[1:])):
        raise ValueError(f"reduced-density key {k}: the sites must be non-decreasing")
    legs = [0] * nsite
    for s in k:
        legs[s] += 1
        if legs[s] > 2:
            raise ValueError(f"reduced-density key {k}: site {s} appears {k.count(s)} times, a site is named once (diagonal) "
                             "or twice (ket and bra)")
    return legs


def pair_key(key, nsite: int) -> tuple[int, int]:
    """The bond of a pair channel, ``(q, q + 1)`` with ``0 <= q < nsite - 1``, from a key given as a tuple;
    ``ValueError`` naming the key otherwise (not two sites, not neighbours, descending, out of range).  Pure Python."""
    try:
        k = tuple(int(s) for s in key)
    except TypeError:
        raise ValueError(f"pair channel key {key!r}: a key is a tuple of two neighbouring sites (q, q + 1)") from None
    if len(k) != 2:
        raise ValueError(f"pair channel key {k}: a key names two neighbouring sites (q, q + 1)")
    if k[1] != k[0] + 1:
        raise ValueError(f"pair channel key {k}: the sites must be nearest neighbours in ascending order, (q, q + 1)")
    if not 0 <= k[0] < nsite - 1:
        raise ValueError(f"pair channel key {k}: bond out of range (the chain has {nsite} sites)")
    return k


def spectra_bonds(bonds, nsite: int) -> list[int]:
    """The bond list of a spectra request as plain integers: an iterable of whole numbers (a single number is a list of
    one).  ``ValueError`` for anything that is not a whole number or does not fit the library's ``int``; range and order
    are the library's to check (``mitdvp_batch_set_spectra``), whose message names the limit.  Pure Python."""
    import numbers

    if isinstance(bonds, numbers.Integral):
        bonds = [bonds]
    try:
        items = list(bonds)
    except TypeError:
        raise ValueError(f"spectra bonds {bonds!r}: a list of bonds q, 0 <= q <= {nsite - 2}") from None
    out = []
    for q in items:
        if isinstance(q, bool) or not isinstance(q, (numbers.Integral, np.integer)):
            raise ValueError(f"spectra bonds {items!r}: bond {q!r} is not a whole number (bond q lies between sites q and q + 1)")
        if not -2**31 <= int(q) < 2**31:
            raise ValueError(f"spectra bonds {items!r}: bond {q!r} does not fit an int")
        out.append(int(q))
    return out


def expect_ops(op_ids) -> list[int]:
    """The operator list of an expect request as plain integers: an iterable of whole numbers (a single number is a list
    of one).  ``ValueError`` for anything that is not a whole number, is negative, does not fit the library's ``int`` or
    is listed twice, and for more than 64 operators; whether every replica carries the operators, and their shapes, are the
    library's to check (``mitdvp_batch_set_expect``), whose message names the operator, the site and the limit.  Pure
    Python."""
    import numbers

    if isinstance(op_ids, numbers.Integral) and not isinstance(op_ids, bool):
        op_ids = [op_ids]
    try:
        items = list(op_ids)
    except TypeError:
        raise ValueError(f"expect operators {op_ids!r}: a list of operator ids (the op_id of set_mpo)") from None
    out = []
    for k in items:
        if isinstance(k, bool) or not isinstance(k, (numbers.Integral, np.integer)):
            raise ValueError(f"expect operators {items!r}: operator {k!r} is not a whole number")
        if not 0 <= int(k) < 2**31:
            raise ValueError(f"expect operators {items!r}: operator {k!r} is negative or does not fit an int")
        if int(k) in out:
            raise ValueError(f"expect operators {items!r}: operator {k!r} is listed twice")
        out.append(int(k))
    if len(out) > 64:
        raise ValueError(f"expect operators: {len(out)} operators, a request takes at most 64")
    return out


def sample_request(nshots, seed=0) -> tuple[int, int]:
    """``nshots`` and ``seed`` of a samples request as plain integers.  ``ValueError`` for anything that is not a whole
    number or does not fit the library's ``int`` / 64-bit unsigned seed; the range of ``nshots`` is the library's to check
    (``mitdvp_batch_set_samples``), whose message names the limit.  Pure Python."""
    import numbers

    for name, x in (("nshots", nshots), ("seed", seed)):
        if isinstance(x, bool) or not isinstance(x, (numbers.Integral, np.integer)):
            raise ValueError(f"samples request: {name} = {x!r} is not a whole number")
    if not -2**31 <= int(nshots) < 2**31:
        raise ValueError(f"samples request: nshots = {nshots!r} does not fit an int")
    if not 0 <= int(seed) < 2**64:
        raise ValueError(f"samples request: seed = {seed!r} is not a 64-bit unsigned number")
    return int(nshots), int(seed)


def operate_request(n_replicas, op_id=0, maxstep=10, conv_tol=1.0e-8, replicas=None):
    """The arguments of ``TDVPBatch.operate`` as plain numbers: ``(op_id, maxstep, conv_tol, replicas)`` with ``replicas``
    a list of distinct replica indices or ``None`` for all ``n_replicas``.  ``ValueError`` naming the argument and the
    limit for an ``op_id`` or ``maxstep`` that is not a whole number or does not fit the library's ``int``, a negative
    ``op_id``, ``maxstep < 1``, a ``conv_tol`` that is not a number, is negative or not finite, and a replica that is not
    a whole number, is outside ``0 .. n_replicas - 1`` or is listed twice; an empty list selects nothing and is refused
    too.  Whether the replicas carry the operator, and its shapes, are the library's to check
    (``mitdvp_batch_operate``).  Pure Python."""
    import math
    import numbers

    def whole(name, x):
        if isinstance(x, bool) or not isinstance(x, (numbers.Integral, np.integer)):
            raise ValueError(f"operate: {name} = {x!r} is not a whole number")
        if not -2**31 <= int(x) < 2**31:
            raise ValueError(f"operate: {name} = {x!r} does not fit an int")
        return int(x)

    op_id, maxstep = whole("op_id", op_id), whole("maxstep", maxstep)
    if op_id < 0:
        raise ValueError(f"operate: op_id = {op_id} is negative (operator ids are >= 0)")
    if maxstep < 1:
        raise ValueError(f"operate: maxstep = {maxstep}, it must be >= 1")
    if isinstance(conv_tol, bool) or not isinstance(conv_tol, (numbers.Real, np.floating, np.integer)):
        raise ValueError(f"operate: conv_tol = {conv_tol!r} is not a number")
    conv_tol = float(conv_tol)
    if not math.isfinite(conv_tol) or conv_tol < 0.0:
        raise ValueError(f"operate: conv_tol = {conv_tol!r}, it must be finite and >= 0")
    if replicas is None:
        return op_id, maxstep, conv_tol, None
    if isinstance(replicas, (numbers.Integral, np.integer)) and not isinstance(replicas, bool):
        replicas = [replicas]
    try:
        items = list(replicas)
    except TypeError:
        raise ValueError(f"operate: replicas = {replicas!r}: a list of replica indices, or None for all") from None
    if not items:
        raise ValueError("operate: replicas is empty (None selects all)")
    out = []
    for r in items:
        r = whole("replica", r)
        if not 0 <= r < n_replicas:
            raise ValueError(f"operate: replica {r} is outside 0 .. {n_replicas - 1}")
        if r in out:
            raise ValueError(f"operate: replica {r} is listed twice")
        out.append(r)
    return op_id, maxstep, conv_tol, out


def field_request(fields, dims, n_replicas):
    """The table of ``TDVPBatch.set_fields`` as what the library takes: ``{site: (V, g, kind, table, sigma, tau)}`` with
    ``G = V diag(g) V^+`` by ``numpy.linalg.eigh``, ``table`` a ``(n,)`` or ``(n_replicas, n)`` array of doubles for a
    pulse and ``None`` for noise.  ``fields``: ``{site: dict(G=(d, d) Hermitian, pulse=array (n,) | (B, n))}`` or
    ``dict(G=..., sigma=s, tau=t)``; ``None`` or ``{}`` is no field.  ``ValueError`` naming the site and what is wrong for
    a site out of range, a ``G`` that is not square, not Hermitian (``|G - G^+|`` above ``1e-12 |G|``) or not of the
    site's order ``dims[site]``, an unknown key, both ``pulse`` and ``sigma`` or neither, a pulse that is not ``(n,)`` or
    ``(n_replicas, n)`` with ``n >= 1`` finite real numbers, and a ``sigma`` or ``tau`` that is negative or not finite.
    Pure Python."""
    out = {}
    for site, spec in dict(fields or {}).items():
        if isinstance(site, bool) or not isinstance(site, (int, np.integer)) or not 0 <= int(site) < len(dims):
            raise ValueError(f"fields: site {site!r} is out of range (the chain has sites 0 .. {len(dims) - 1})")
        site = int(site)
        who = f"fields[{site}]"
        if not isinstance(spec, dict) or "G" not in spec:
            raise ValueError(f"{who} must be dict(G=..., pulse=...) or dict(G=..., sigma=..., tau=...)")
        unknown = sorted(set(spec) - {"G", "pulse", "sigma", "tau"})
        if unknown:
            raise ValueError(f"{who}: unknown key {unknown[0]!r} (G, pulse, sigma, tau)")
        G = np.asarray(spec["G"], dtype=np.complex128)
        if G.ndim != 2 or G.shape[0] != G.shape[1]:
            raise ValueError(f"{who}: G must be a square matrix, got shape {G.shape}")
        if G.shape[0] != dims[site]:
            raise ValueError(f"{who}: G is of order {G.shape[0]}, the site's physical dimension is {dims[site]}")
        if not np.all(np.isfinite(G)) or np.linalg.norm(G - G.conj().T) > 1e-12 * np.linalg.norm(G):
            raise ValueError(f"{who}: G is not Hermitian (|G - G^+| = {np.linalg.norm(G - G.conj().T):.3e}, |G| = "
                             f"{np.linalg.norm(G):.3e})")
        has_pulse, has_noise = spec.get("pulse") is not None, spec.get("sigma") is not None
        if has_pulse == has_noise:
            raise ValueError(f"{who}: give either pulse (a table of amplitudes) or sigma and tau (noise), "
                             f"{'not both' if has_pulse else 'one of them'}")
        g, V = np.linalg.eigh(0.5 * (G + G.conj().T))
        V, g = np.ascontiguousarray(V, dtype=np.complex128), np.ascontiguousarray(g, dtype=np.float64)
        if has_pulse:
            if "tau" in spec and spec["tau"] is not None:
                raise ValueError(f"{who}: tau goes with sigma (noise), not with pulse")
            tab = np.asarray(spec["pulse"])
            if np.iscomplexobj(tab) or tab.dtype == object:
                raise ValueError(f"{who}: pulse must be real numbers")
            tab = np.ascontiguousarray(tab, dtype=np.float64)
            if tab.ndim not in (1, 2) or tab.shape[-1] < 1 or (tab.ndim == 2 and tab.shape[0] != n_replicas):
                raise ValueError(f"{who}: pulse must have shape (n,) or ({n_replicas}, n) with n >= 1 -- one row per replica; "
                                 f"got {tab.shape}")
            if not np.all(np.isfinite(tab)):
                raise ValueError(f"{who}: pulse must be finite numbers")
            out[site] = (V, g, _lib.FIELD_TABLE, tab, 0.0, 0.0)
        else:
            try:
                sigma, tau = float(spec["sigma"]), float(spec.get("tau") or 0.0)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: sigma and tau must be numbers") from None
            if not (np.isfinite(sigma) and sigma >= 0.0 and np.isfinite(tau) and tau >= 0.0):
                raise ValueError(f"{who}: sigma = {sigma!r} and tau = {tau!r} must be finite and >= 0")
            out[site] = (V, g, _lib.FIELD_OU, None, sigma, tau)
    return out


class TDVPBatch:
    """B independent trajectories (replicas) of one chain shape on ONE GPU, any B: one kernel launch per half-sweep for the
    whole batch (``mitdvp_batch_step`` / ``k_batch_sweep``: one workgroup owns one replica, the replica index is the
    workgroup index).  Unlike ``TDVPEnsemble`` there are no compute-unit ranges, no host threads and no limit of 16
    replicas; the replicas are ordinary full-device engines (``engines``), usable on their own between batch calls, and
    ``from_engines`` takes engines that each carry their own MPO.  Shapes must be inside the kernel's envelope
    (dl*d*dr <= 8192 per site, MPO bonds <= 16) and equal across replicas, as must the integrator settings.

    ``propagate`` raises the first failing replica's error (a replica that does not converge stops, the others finish)
    and leaves every replica's status code in ``statuses``.

    With ``relax="improved"`` (and ``from_engines`` of such engines) the batch finds ground states: every half-sweep
    replaces each site tensor by the lowest eigenvector of its effective Hamiltonian (``k_batch_relax``; a Lanczos solver
    that stays on the device) and skips the bond step.  ``propagate``, ``sweep`` and ``propagate(observe=...)`` work as
    ever, two launches per step; their ``dt_au`` means nothing there, as for ``TDVPEngine(relax="improved")``.  ``relax``
    runs many steps in one launch and stops each replica when its energy has converged.  A local solve takes at most
    ``max_diag_krylov`` <= 64 vectors; ``set_relax_restarts`` lets it restart from its lowest Ritz vector instead of
    giving up there.
    """

    def __init__(self, n_replicas: int, nsite: int, *, device: int = 0, **engine_kw):
        if n_replicas < 1:
            raise ValueError("n_replicas must be >= 1")
        if "cu_range" in engine_kw:
            raise ValueError("TDVPBatch replicas run on the whole device: no cu_range")
        self.engines = []
        self._own = True
        self._b = None
        self._key = None
        self.statuses = []
        self.records = {}
        self._channels = {}
        self._fields = {}
        self._seed = None
        self._cross = None
        self._spectra = None
        self._samples = None
        self._expect = None
        self._cross_mpo = None
        self.operated = {}
        self.relaxed = {}
        self._restarts = None
        self._lib = _lib.load()
        try:
            for _ in range(n_replicas):
                self.engines.append(TDVPEngine(nsite, device=device, **engine_kw))
        except Exception:
            self.close()
            raise

    @classmethod
    def from_engines(cls, engines):
        """A batch over existing engines (each with its own MPO and state); ``close`` leaves them open."""
        engines = list(engines)
        if not engines:
            raise ValueError("n_replicas must be >= 1")
        self = cls.__new__(cls)
        self.engines = engines
        self._own = False
        self._b = None
        self._key = None
        self.statuses = []
        self.records = {}
        self._channels = {}
        self._fields = {}
        self._seed = None
        self._cross = None
        self._spectra = None
        self._samples = None
        self._expect = None
        self._cross_mpo = None
        self.operated = {}
        self.relaxed = {}
        self._restarts = None
        self._lib = _lib.load()
        return self

    def __len__(self):
        return len(self.engines)

    def __getitem__(self, i):
        return self.engines[i]

    def set_mpo(self, cores, op_id: int = 0):
        for e in self.engines:
            e.set_mpo(cores, op_id)

    def _handle(self):
        # created at the first step (the engines get their tensors and MPOs after construction) and again when the list
        # of engines changed; the library validates the replicas at creation and at every step
        key = tuple(e._h.value if hasattr(e._h, "value") else e._h for e in self.engines)
        if self._b is None or key != self._key:
            self._drop()
            n = len(self.engines)
            hs = (C.c_void_p * n)(*[e._h for e in self.engines])
            b = C.c_void_p()
            _lib.check(self._lib.mitdvp_batch_create(hs, n, C.byref(b)))
            self._b, self._key = b, key
            try:  # a handle made anew (the list of engines changed) gets the channels again and counts steps from 0
                for site, (kind, ops) in self._channels.items():
                    self._push_channel(site, kind, ops)
                if self._seed is not None:
                    seed, ids = self._seed
                    if ids is not None and len(ids) != n:  # the library reads one id per replica
                        raise ValueError(f"the batch has {n} replicas now, trajectory_ids were given for {len(ids)}: "
                                         "call set_jumps again")
                    self._push_seed(seed, ids)
                for site, spec in self._fields.items():
                    if spec[3] is not None and spec[3].ndim == 2 and spec[3].shape[0] != n:  # the library reads one row per replica
                        raise ValueError(f"the batch has {n} replicas now, the pulse of site {site} has {spec[3].shape[0]} rows: "
                                         "call set_fields again")
                    self._push_field(site, spec)
                if self._cross is not None:  # the new handle has no snapshot: a request that names one is refused here
                    self._push_cross(self._cross)
                if self._spectra is not None:
                    self._push_spectra(self._spectra)
                if self._samples is not None:
                    self._push_samples(*self._samples)
                if self._expect is not None:
                    self._push_expect(self._expect)
                if self._cross_mpo is not None:
                    self._push_cross_mpo(self._cross_mpo)
                if self._restarts is not None:
                    _lib.check(self._lib.mitdvp_batch_set_relax_restarts(self._b, self._restarts))
            except Exception:
                self._drop()
                raise
        return self._b

    # ---- one-site channels between the two half-sweeps of a time step (mitdvp_batch_set_channel) ----
    def _push_channel(self, site, kind, ops):
        if isinstance(site, tuple):  # a pair channel on the bond (q, q + 1); ops (K, d0, d1, d0, d1)
            if ops is None:
                _lib.check(self._lib.mitdvp_batch_set_pair_channel(self._b, site[0], 0, None, 0, 0, 0))
            else:
                _lib.check(self._lib.mitdvp_batch_set_pair_channel(self._b, site[0], kind, _dp(ops), ops.shape[0], ops.shape[1],
                                                                   ops.shape[2]))
        elif ops is None:
            _lib.check(self._lib.mitdvp_batch_set_channel(self._b, int(site), 0, None, 0, 0))
        else:
            _lib.check(self._lib.mitdvp_batch_set_channel(self._b, int(site), kind, _dp(ops), ops.shape[0], ops.shape[1]))

    def _pair_ops(self, kind, key, ops):
        """the operators of a pair channel as (K, d0, d1, d0, d1) from (dd, dd) / (K, dd, dd) or the four-leg forms"""
        q = key[0]
        gate = kind == _lib.CHANNEL_GATE
        if gate and ops.ndim in (2, 4):
            ops = ops[None]
        if ops.ndim == 5:
            if ops.shape[1:3] != ops.shape[3:5]:
                raise ValueError(f"bond {key}: four-leg operators are (d0, d1, d0, d1), got shape {ops.shape[1:]}")
            return np.ascontiguousarray(ops)
        if ops.ndim != 3 or ops.shape[1] != ops.shape[2]:
            raise ValueError(f"bond {key}: the operators must be square matrices of order d0 d1 or four-leg tensors "
                             f"(d0, d1, d0, d1); got shape {ops.shape}")
        d0, d1 = (self.engines[0].get_site_shape(p)[1] for p in key)
        if ops.shape[1] != d0 * d1:
            raise ValueError(f"bond {key}: the operators are of order {ops.shape[1]}, the sites' physical dimensions are "
                             f"{d0} x {d1} (order {d0 * d1})")
        return np.ascontiguousarray(ops.reshape(ops.shape[0], d0, d1, d0, d1))

    def _push_seed(self, seed, ids):
        arr = None if ids is None else (C.c_uint64 * len(ids))(*ids)
        _lib.check(self._lib.mitdvp_batch_set_seed(self._b, C.c_uint64(seed), arr))

    def _set_channels(self, kind, table):
        """``table``: {site: operators (K, d, d) or None}.  The library validates; a refused table changes nothing."""
        new = {}
        for site, ops in dict(table).items():
            if isinstance(site, (tuple, list)):
                key = pair_key(site, self.engines[0].nsite)
                new[key] = (kind, None if ops is None else self._pair_ops(kind, key, _c128(ops)))
                continue
            if ops is not None:
                ops = _c128(ops)
                if kind == _lib.CHANNEL_GATE and ops.ndim == 1:  # a diagonal gate, as TDVPEngine.set_gates takes it
                    ops = np.diag(ops)
                if kind == _lib.CHANNEL_GATE and ops.ndim == 2:
                    ops = ops[None]
                if ops.ndim != 3 or ops.shape[1] != ops.shape[2]:
                    raise ValueError(f"site {site}: the operators must be square matrices, (K, d, d); got shape {ops.shape}")
                ops = np.ascontiguousarray(ops)
            new[int(site)] = (kind, ops)
        self._handle()
        done = []
        try:
            for site, (k, ops) in new.items():
                self._push_channel(site, k, ops)
                done.append(site)
        except Exception:
            for site in done:  # back to what was set before
                self._push_channel(site, *self._channels.get(site, (0, None)))
            raise
        for site, (k, ops) in new.items():
            if ops is None:
                self._channels.pop(site, None)
            else:
                self._channels[site] = (k, ops)

    def set_gates(self, gates: dict):
        """``{site: U (d, d) or a length-d diagonal}``: one-site gates applied to every replica between the two half-sweeps of each time step
        (the reference's ``one_gate_to_apply``), as they are -- ``U`` need not be unitary.  ``{site: None}`` removes a
        site's channel.  One more launch per time step while any channel is set.  The replicas must have their tensors
        and MPOs already (the library checks the physical dimensions).

        A key may be a bond ``(q, q + 1)``: a two-site gate ``(d0 d1, d0 d1)``, row-major over the two physical indices, or
        ``(d0, d1, d0, d1)``.  It is applied to the merged two-site tensor, which is split again at the bond's dimension
        as it is (``k_batch_pair``); nothing is rescaled, what the split discards adds to ``discarded_weight()``."""
        self._set_channels(_lib.CHANNEL_GATE, gates)

    def set_jumps(self, jumps: dict, seed: int = 0, trajectory_ids=None):
        """``{site: B (K, d, d)}``, 2 <= K <= 16: a Kraus channel per site unravelled into quantum jumps -- at every time
        step each replica picks ONE operator k with probability |B_k psi|^2 / sum_k |B_k psi|^2 and keeps its norm.  The
        uniforms are ``trajectories.jump_uniform(seed, trajectory_id, step, site)``; ``trajectory_ids`` (default
        0 .. B-1) name the replicas, so a chunked ensemble draws what one big batch draws.  Sets the seed: the step
        counter and ``jump_counts()`` start again from zero.  ``{site: None}`` removes a site's channel.

        The step counter and the jump counters live in the library's batch object.  That object is made anew when the
        list ``engines`` is changed between calls (an engine replaced, added or taken out); the channels and the seed
        are then set again on the new one, so the step counter and the jump counters start again from zero in the
        middle of an ensemble, and ``trajectory_ids`` given for another number of replicas raise ``ValueError`` until
        ``set_jumps`` is called again.

        A key may be a bond ``(q, q + 1)`` with ``B`` of shape ``(K, d0 d1, d0 d1)`` or ``(K, d0, d1, d0, d1)``: the same
        rule on the merged two-site tensor with the uniform ``jump_uniform(seed, trajectory_id, step, L + q)``; the norm
        after the re-split equals the norm before the jump.  Counted in ``pair_jump_counts()``."""
        n = len(self.engines)
        ids = None
        if trajectory_ids is not None:
            ids = [int(t) for t in trajectory_ids]
            if len(ids) != n or any(not 0 <= t < 2**64 for t in ids):
                raise ValueError(f"trajectory_ids must be {n} integers in [0, 2^64), one per replica")
        seed = int(seed)
        if not 0 <= seed < 2**64:
            raise ValueError("seed must be in [0, 2^64)")
        stale, made = self._seed, self._b
        self._seed = (seed, ids)  # a batch object made anew inside this call gets these ids, not the ones of before
        try:
            self._set_channels(_lib.CHANNEL_JUMP, jumps)
            self._push_seed(seed, ids)
        except Exception:
            self._seed = stale
            if self._b is not made:  # made anew with the seed that was refused: the next call makes it again
                self._drop()
            raise

    def jump_counts(self):
        """(B, L, 16) integers: how often operator k of site p's jump channel was picked by replica r since the seed
        was set; zeros where no jump channel acts.  They start again from zero with every ``set_jumps`` and when the
        list ``engines`` was changed since the last call (see ``set_jumps``)."""
        n, nsite = len(self.engines), self.engines[0].nsite
        out = np.zeros((n, nsite, _lib.MAX_JUMP), dtype=np.int64)
        _lib.check(self._lib.mitdvp_batch_jump_counts(self._handle(), out.ctypes.data_as(C.POINTER(C.c_longlong))))
        return out

    def pair_jump_counts(self):
        """(B, L, 16) integers: how often operator k of the pair jump channel on bond (q, q + 1) -- row q -- was picked by
        replica r since the seed was set; they start again from zero when ``jump_counts()`` does."""
        n, nsite = len(self.engines), self.engines[0].nsite
        out = np.zeros((n, nsite, _lib.MAX_JUMP), dtype=np.int64)
        _lib.check(self._lib.mitdvp_batch_pair_jump_counts(self._handle(), out.ctypes.data_as(C.POINTER(C.c_longlong))))
        return out

    def discarded_weight(self):
        """(B,) numbers: per replica the sum over the splits of its pair channels of the weight each split discarded,
        ``sum_{j>r} sigma_j^2 / sum_j sigma_j^2`` (r: the bond's dimension), since the seed or a channel was last set."""
        out = np.zeros(len(self.engines), dtype=np.float64)
        _lib.check(self._lib.mitdvp_batch_discarded_weight(self._handle(), _dp(out)))
        return out

    # ---- time-dependent one-site fields between the half-sweeps (mitdvp_batch_set_field) ----
    def _push_field(self, site, spec):
        if spec is None:
            _lib.check(self._lib.mitdvp_batch_set_field(self._b, int(site), 0, None, None, 0, None, 0, 0, 0.0, 0.0))
            return
        V, g, kind, tab, sigma, tau = spec
        ntab, per = (0, 0) if tab is None else (tab.shape[-1], int(tab.ndim == 2))
        _lib.check(self._lib.mitdvp_batch_set_field(self._b, int(site), V.shape[0], _dp(V), _dp(g), kind,
                                                    None if tab is None else _dp(tab), ntab, per, sigma, tau))

    def set_fields(self, fields):
        """Time-dependent one-site terms ``H(t) = H0 + sum_p a_p(t) G_p`` for every replica: ``fields`` maps a site to
        ``dict(G=(d, d) Hermitian, pulse=array (n,) | (B, n))`` -- ``a_p`` of the n-th time step since this call (or the
        last ``set_jumps``, which sets the seed) is ``pulse[n]``, the same for all replicas or one row per replica, and 0
        once the table is used up; give midpoint values (``trajectories.pulse_table``) -- or to
        ``dict(G=..., sigma=s, tau=t)``: a stationary Ornstein-Uhlenbeck process per (trajectory, site) of standard
        deviation ``s`` and correlation time ``t`` (the unit of ``dt_au``; 0: white noise), the numbers of
        ``trajectories.field_noise_path`` under the seed and ids of ``set_jumps``.  The table REPLACES the fields set
        before; ``{}`` or ``None`` removes them all.  Amplitude times ``G`` is in the Hamiltonian's unit.

        Each term acts as the one-site unitary ``exp(-i dt a_p G_p)`` between the two half-sweeps of a time step
        (``k_batch_field``, one more launch per step while a field is set), before the gates and jump channels; the step
        is accurate to O(dt^2).  ``G`` is diagonalised here (``numpy.linalg.eigh``).  ``ValueError`` before the library
        is touched for what ``field_request`` refuses; the library refuses a site of physical dimension above 64 and
        replicas in imaginary time.  The fields are set again on a library object made anew (see ``set_jumps``)."""
        n = len(self.engines)
        dims = [self.engines[0].get_site_shape(p)[1] for p in range(self.engines[0].nsite)]
        new = field_request(fields, dims, n)
        self._handle()
        old = self._fields
        try:
            for site in old:
                if site not in new:
                    self._push_field(site, None)
            for site, spec in new.items():
                self._push_field(site, spec)
        except Exception:
            for site in set(old) | set(new):  # back to what was set before
                self._push_field(site, old.get(site))
            raise
        self._fields = new

    def field_values(self):
        """(B, L) numbers: the amplitude ``a_p`` every replica applied on every site in the last time step, 0 where no
        field acted."""
        out = np.zeros((len(self.engines), self.engines[0].nsite), dtype=np.float64)
        _lib.check(self._lib.mitdvp_batch_field_values(self._handle(), _dp(out)))
        return out

    # ---- cross overlaps and one-site matrix elements between replicas (mitdvp_batch_set_cross / _cross) ----
    def snap(self, r: int) -> int:
        """the state index of the snapshot of replica ``r``, for ``set_cross``"""
        n = len(self.engines)
        if not 0 <= int(r) < n:
            raise ValueError(f"snap: replica {r} is out of range (the batch has {n})")
        return n + int(r)

    def snapshot(self):
        """Copies every site tensor of every replica into a device buffer of the batch by ONE launch
        (``mitdvp_batch_snapshot``); ``snap(r)`` then names that copy of replica ``r`` in ``set_cross``.  The centre may be
        at site 0 or at the last site.  A snapshot stays until the next one; it is lost, with the library's batch object,
        when the list ``engines`` is changed."""
        _lib.check(self._lib.mitdvp_batch_snapshot(self._handle()))

    def _push_cross(self, packed):
        bra, ket, site, ops, dims = packed
        n = len(bra)
        ia = lambda v: (C.c_int * max(len(v), 1))(*v)
        _lib.check(self._lib.mitdvp_batch_set_cross(self._b, n, ia(bra), ia(ket), ia(site), _dp(ops) if ops.size else None, ia(dims)))

    def set_cross(self, entries):
        """Registers the pairs that ``cross`` and recorded runs evaluate: an entry is ``(bra, ket)`` -- the overlap
        ``<psi_bra|psi_ket>`` -- or ``(bra, ket, site, O)`` -- ``<psi_bra| O_site |psi_ket>`` with ``O`` a ``(d, d)``
        matrix, need not be Hermitian.  ``bra`` / ``ket`` are replica indices or ``snap(r)``.  An empty list removes the
        request.  The library validates (indices, a snapshot that exists, the site, the operator's order, at most 65536
        pairs) and a refused request leaves the one before in place."""
        bra, ket, site, ops, dims = [], [], [], [], []
        for k, e in enumerate(entries):
            e = tuple(e)
            if len(e) == 2:
                e = (e[0], e[1], -1, None)
            if len(e) != 4 or (e[3] is None) != (int(e[2]) == -1):
                raise ValueError(f"set_cross: entry {k} must be (bra, ket) or (bra, ket, site, O)")
            bra.append(int(e[0])); ket.append(int(e[1])); site.append(int(e[2]))
            if e[3] is not None:
                O = _c128(e[3])
                if O.ndim != 2 or O.shape[0] != O.shape[1]:
                    raise ValueError(f"set_cross: entry {k}: the operator must be a square matrix, got shape {O.shape}")
                ops.append(O.ravel())
                dims.append(O.shape[0])
        packed = (bra, ket, site, np.ascontiguousarray(np.concatenate(ops)) if ops else np.zeros(0, dtype=np.complex128), dims)
        self._handle()
        self._push_cross(packed)
        self._cross = packed if bra else None

    def _request_weights(self, name, unit, weights):
        """The weights of request ``name`` ("cross", "spectra", "samples", "expect", "cross_mpo") as a float64 array, or
        None for the default.  ``unit`` says what one weight multiplies, and with it how many are expected: "replica", one
        per replica, or an item of the request's first list ("pair", "entry").  ValueError when the request is not set or
        the count is wrong."""
        req = getattr(self, "_" + name)
        if req is None:
            title = "cross request of MPOs" if name == "cross_mpo" else f"{name} request"
            raise ValueError(f"no {title} is set (set_{name})")
        if weights is None:
            return None
        count = len(self.engines) if unit == "replica" else len(req[0])
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
        if w.shape != (count,):
            raise ValueError(f"{name} weights must be {count} numbers, one per {unit} (got shape {w.shape})")
        return w

    def cross(self, weights=None):
        """The request of ``set_cross`` on the current state of the replicas: one launch for all pairs, a second one for
        their weighted sum (``mitdvp_batch_cross``).  Returns ``{"values": (P,) complex, "mean": complex}``; ``weights``:
        P numbers, default 1 / P each."""
        w = self._request_weights("cross", "pair", weights)
        vals = np.zeros(len(self._cross[0]), dtype=np.complex128)
        mean = np.zeros(1, dtype=np.complex128)
        _lib.check(self._lib.mitdvp_batch_cross(self._handle(), None if w is None else _dp(w), _dp(vals), _dp(mean)))
        return {"values": vals, "mean": complex(mean[0])}

    def _cross_records(self, weights):
        w = self._request_weights("cross", "pair", weights)
        cnt = (C.c_size_t * 2)()
        _lib.check(self._lib.mitdvp_batch_cross_records(self._b, None, None, None, cnt))
        nrec, npairs = int(cnt[0]), int(cnt[1])
        vals = np.zeros((nrec, npairs), dtype=np.complex128)
        mean = np.zeros(nrec, dtype=np.complex128)
        _lib.check(self._lib.mitdvp_batch_cross_records(self._b, None if w is None else _dp(w), _dp(vals), _dp(mean), cnt))
        return vals, mean

    # ---- bond spectra and entanglement entropies (mitdvp_batch_set_spectra / _spectra) ----
    def _push_spectra(self, bonds):
        arr = (C.c_int * max(len(bonds), 1))(*bonds)
        _lib.check(self._lib.mitdvp_batch_set_spectra(self._b, arr, len(bonds)))

    def set_spectra(self, bonds):
        """Registers the bonds whose Schmidt spectra ``spectra`` and recorded runs evaluate: a strictly ascending list of
        bonds ``q`` in ``0 .. L-2``; bond ``q`` lies between sites ``q`` and ``q + 1``.  An empty list removes the
        request.  The library validates (range, order, the record's size) and a refused request leaves the one before
        in place."""
        bonds = spectra_bonds(bonds, self.engines[0].nsite)
        self._handle()
        self._push_spectra(bonds)
        self._spectra = bonds if bonds else None

    def _split_spectra(self, values, mean, per_replica=True):
        """the flat records cut by bond: W, S1, S2, pmin and the chi weights of every requested bond"""
        chis = [self.engines[0].get_site_shape(q)[2] for q in self._spectra]
        res = {}
        for prefix, flat in (("mean_", mean), ("", values)):
            if flat is None or (not prefix and not per_replica):
                continue
            head, wts, at = [], [], 0
            for chi in chis:
                head.append(flat[..., at:at + 4])
                wts.append(np.ascontiguousarray(flat[..., at + 4:at + 4 + chi]))
                at += 4 + chi
            head = np.stack(head, axis=-2)  # (..., nb, 4)
            for k, name in enumerate(("norm2", "entropy", "renyi2", "min_weight")):
                res[prefix + name] = np.ascontiguousarray(head[..., k])
            res[prefix + "weights"] = wts
        return res

    def spectra(self, weights=None, per_replica: bool = True):
        """The Schmidt spectrum of every bond of ``set_spectra`` for every replica by ONE launch (``k_batch_spectra``), the
        ensemble means by a second one (``mitdvp_batch_spectra``); all replicas must have their centre at site 0 and are
        only read.  Returns, with ``nb`` the number of requested bonds: ``mean_entropy`` (von Neumann, natural
        logarithm), ``mean_renyi2``, ``mean_min_weight`` (the smallest normalised Schmidt weight: how close the bond is
        to being too narrow), ``mean_norm2``, each ``(nb,)``; ``mean_weights``, a list of ``(chi_q,)`` arrays of squared
        Schmidt values, descending, not normalised; and, with ``per_replica``, the same names without ``mean_`` and with
        a leading B axis.  The entropies are those of each trajectory, THEN averaged: they are not functions of the
        averaged densities.  ``weights``: B numbers, default 1 / B each."""
        w = self._request_weights("spectra", "replica", weights)
        b = self._handle()
        cnt = (C.c_size_t * 2)()
        _lib.check(self._lib.mitdvp_batch_spectra(b, None, None, None, cnt))
        n, rec_len = int(cnt[0]), int(cnt[1])
        vals = np.zeros((n, rec_len), dtype=np.float64)
        mean = np.zeros(rec_len, dtype=np.float64)
        _lib.check(self._lib.mitdvp_batch_spectra(b, None if w is None else _dp(w), _dp(vals), _dp(mean), cnt))
        return self._split_spectra(vals, mean, per_replica)

    def _spectra_records(self, weights, per_replica=True):
        w = self._request_weights("spectra", "replica", weights)
        cnt = (C.c_size_t * 3)()
        _lib.check(self._lib.mitdvp_batch_spectra_records(self._b, None, None, None, cnt))
        nrec, n, rec_len = (int(c) for c in cnt)
        vals = np.zeros((nrec, n, rec_len), dtype=np.float64)
        mean = np.zeros((nrec, rec_len), dtype=np.float64)
        _lib.check(self._lib.mitdvp_batch_spectra_records(self._b, None if w is None else _dp(w), _dp(vals), _dp(mean), cnt))
        return self._split_spectra(vals, mean, per_replica)

    # ---- sampled configurations (mitdvp_batch_set_samples / _samples) ----
    def _push_samples(self, nshots, seed):
        _lib.check(self._lib.mitdvp_batch_set_samples(self._b, nshots, C.c_ulonglong(seed)))

    def set_samples(self, nshots, seed=0):
        """Registers the request that ``samples`` and recorded runs evaluate: ``nshots`` configurations of every replica,
        drawn with the counter-based uniforms ``trajectories.sample_uniform(seed, trajectory_id, step, site, shot)``;
        ``nshots = 0`` removes the request.  The library validates the range (at most 65 536 shots, ``nshots * L`` at most
        2^22) and a refused request leaves the one before in place."""
        nshots, seed = sample_request(nshots, seed)
        self._handle()
        self._push_samples(nshots, seed)
        self._samples = (nshots, seed) if nshots else None

    def _split_samples(self, configs, prob, freq, mean, per_replica=True):
        """the flat frequency axis cut by site: one (.., d_p) array per site"""
        dims = [self.engines[0].get_site_shape(p)[1] for p in range(self.engines[0].nsite)]
        cut = lambda flat: [np.ascontiguousarray(flat[..., at - d:at]) for d, at in zip(dims, np.cumsum(dims))]
        res = {"mean_freq": cut(mean)}
        if per_replica:
            res.update(configs=configs, prob=prob, freq=cut(freq))
        return res

    def _samples_call(self, fn, w, nlead, per_replica):
        """the size query, the arrays and the call of ``mitdvp_batch_samples`` (``nlead`` = 0) or ``_samples_records``
        (``nlead`` = 1: a leading record axis, counts one entry longer)"""
        ip = C.POINTER(C.c_int)
        cnt = (C.c_size_t * (4 + nlead))()
        _lib.check(fn(self._b, None, None, None, None, None, cnt))
        shape = tuple(int(c) for c in cnt)
        lead, (n, nshots, nsite, F) = shape[:nlead], shape[nlead:]
        mean = np.zeros(lead + (F,), dtype=np.float64)
        configs = prob = freq = None
        if per_replica:
            configs = np.full(lead + (n, nshots, nsite), -1, dtype=np.int32)
            prob = np.zeros(lead + (n, nshots), dtype=np.float64)
            freq = np.zeros(lead + (n, F), dtype=np.float64)
        _lib.check(fn(self._b, None if w is None else _dp(w), None if configs is None else configs.ctypes.data_as(ip),
                      None if prob is None else _dp(prob), None if freq is None else _dp(freq), _dp(mean), cnt))
        return self._split_samples(configs, prob, freq, mean, per_replica)

    def samples(self, weights=None, per_replica: bool = True):
        """``nshots`` configurations of every replica's current state by ONE launch (``k_batch_sample``), the ensemble
        means of their one-site frequencies by a second one (``mitdvp_batch_samples``); all replicas must have their
        centre at site 0 and are only read.  Returns ``mean_freq``, a list of ``(d_p,)`` arrays -- the weighted sum over
        the replicas of the fraction of shots that gave outcome ``j`` at site ``p`` -- and, with ``per_replica``,
        ``configs`` ``(B, nshots, L)`` int32 (one basis index per site; -1 from the site on at which a zero state left no
        weight), ``prob`` ``(B, nshots)`` (``|<config|psi>|^2 / <psi|psi>``) and ``freq``, a list of ``(B, d_p)`` arrays.
        ``weights``: B numbers, default 1 / B each."""
        w = self._request_weights("samples", "replica", weights)
        self._handle()
        return self._samples_call(self._lib.mitdvp_batch_samples, w, 0, per_replica)

    def _samples_records(self, weights, per_replica=True):
        w = self._request_weights("samples", "replica", weights)
        return self._samples_call(self._lib.mitdvp_batch_samples_records, w, 1, per_replica)

    # ---- expectation values of MPO observables (mitdvp_batch_set_expect / _expect) ----
    def _push_expect(self, ops):
        arr = (C.c_int * max(len(ops), 1))(*ops)
        _lib.check(self._lib.mitdvp_batch_set_expect(self._b, arr, len(ops)))

    def set_expect(self, op_ids):
        """Registers the operators whose expectation values ``expect`` and recorded runs evaluate: a list of the
        ``op_id`` under which ``set_mpo`` gave every replica the operator's cores (``TDVPEngine.set_mpo(..., shift=)`` its
        scalar term); 0, the
        Hamiltonian, is allowed.  An empty list removes the request.  The replicas must carry the operators already: the
        library validates (every site, equal shapes across the replicas, MPO bonds of at most 16, outer bonds 1) and a
        refused request leaves the one before in place."""
        ops = expect_ops(op_ids)
        self._handle()
        self._push_expect(ops)
        self._expect = ops if ops else None

    def expect(self, weights=None, per_replica: bool = True):
        """``<psi | O_k | psi> + shift_k <psi | psi>`` (not normalised, as ``TDVPEngine.expectation``) of every operator of
        ``set_expect`` for every replica by ONE launch (``k_batch_expect``, one workgroup per replica and operator), the
        ensemble means by a second one (``mitdvp_batch_expect``); all replicas must have their centre at site 0 and are
        only read.  Returns ``mean`` of shape ``(nops,)`` and, with ``per_replica``, ``values`` ``(B, nops)``, complex, in
        the order of the request.  ``weights``: B numbers, default 1 / B each."""
        w = self._request_weights("expect", "replica", weights)
        b = self._handle()
        cnt = (C.c_size_t * 2)()
        _lib.check(self._lib.mitdvp_batch_expect(b, None, None, None, cnt))
        n, nops = int(cnt[0]), int(cnt[1])
        vals = np.zeros((n, nops), dtype=np.complex128)
        mean = np.zeros(nops, dtype=np.complex128)
        _lib.check(self._lib.mitdvp_batch_expect(b, None if w is None else _dp(w), _dp(vals), _dp(mean), cnt))
        return {"values": vals, "mean": mean} if per_replica else {"mean": mean}

    def _expect_records(self, weights, per_replica=True):
        w = self._request_weights("expect", "replica", weights)
        cnt = (C.c_size_t * 3)()
        _lib.check(self._lib.mitdvp_batch_expect_records(self._b, None, None, None, cnt))
        nrec, n, nops = (int(c) for c in cnt)
        vals = np.zeros((nrec, n, nops), dtype=np.complex128)
        mean = np.zeros((nrec, nops), dtype=np.complex128)
        _lib.check(self._lib.mitdvp_batch_expect_records(self._b, None if w is None else _dp(w), _dp(vals), _dp(mean), cnt))
        return {"expect": vals, "mean_expect": mean} if per_replica else {"mean_expect": mean}

    # ---- MPO matrix elements between replicas (mitdvp_batch_set_cross_mpo / _cross_mpo) ----
    def _push_cross_mpo(self, packed):
        bra, ket, ops = packed
        ia = lambda v: (C.c_int * max(len(v), 1))(*v)
        _lib.check(self._lib.mitdvp_batch_set_cross_mpo(self._b, len(bra), ia(bra), ia(ket), ia(ops)))

    def set_cross_mpo(self, entries):
        """Registers the entries that ``cross_mpo`` and recorded runs evaluate: ``(bra, ket, op_id)`` is
        ``<psi_bra| O |psi_ket> + shift <psi_bra|psi_ket>``, not normalised, with ``O`` the MPO that every replica carries
        under ``op_id`` (``set_mpo``) -- the cores and the scalar term of the ket's owner.  ``bra`` / ``ket`` are replica
        indices or ``snap(r)``.  An empty list removes the request.  The library validates (indices, a snapshot that
        exists, every site, equal shapes across the replicas, MPO bonds of at most 16, outer bonds 1, at most 65536
        entries, a work buffer of at most 2**32 bytes) and a refused request leaves the one before in place."""
        bra, ket, ops = [], [], []
        for k, e in enumerate(entries):
            e = tuple(e)
            if len(e) != 3:
                raise ValueError(f"set_cross_mpo: entry {k} must be (bra, ket, op_id)")
            try:
                e = tuple(operator.index(x) for x in e)
            except TypeError:
                raise ValueError(f"set_cross_mpo: entry {k} must be three whole numbers (bra, ket, op_id), got {e!r}") from None
            if any(not -2**31 <= x < 2**31 for x in e):
                raise ValueError(f"set_cross_mpo: entry {k}: {e!r} does not fit an int")
            bra.append(e[0]); ket.append(e[1]); ops.append(e[2])
        packed = (bra, ket, ops)
        self._handle()
        self._push_cross_mpo(packed)
        self._cross_mpo = packed if bra else None

    def cross_mpo(self, weights=None):
        """The request of ``set_cross_mpo`` on the current state of the replicas: one launch for all entries
        (``k_batch_cross_mpo``, one workgroup per entry), a second one for their weighted sum (``mitdvp_batch_cross_mpo``).
        Returns ``{"values": (P,) complex, "mean": complex}``; ``weights``: P numbers, default 1 / P each."""
        w = self._request_weights("cross_mpo", "entry", weights)
        vals = np.zeros(len(self._cross_mpo[0]), dtype=np.complex128)
        mean = np.zeros(1, dtype=np.complex128)
        _lib.check(self._lib.mitdvp_batch_cross_mpo(self._handle(), None if w is None else _dp(w), _dp(vals), _dp(mean)))
        return {"values": vals, "mean": complex(mean[0])}

    def _cross_mpo_records(self, weights):
        w = self._request_weights("cross_mpo", "entry", weights)
        cnt = (C.c_size_t * 2)()
        _lib.check(self._lib.mitdvp_batch_cross_mpo_records(self._b, None, None, None, cnt))
        nrec, np_ = int(cnt[0]), int(cnt[1])
        vals = np.zeros((nrec, np_), dtype=np.complex128)
        mean = np.zeros(nrec, dtype=np.complex128)
        _lib.check(self._lib.mitdvp_batch_cross_mpo_records(self._b, None if w is None else _dp(w), _dp(vals), _dp(mean), cnt))
        return vals, mean

    # ---- an MPO applied to the replicas (mitdvp_batch_operate) ----
    def operate(self, op_id: int = 0, maxstep: int = 10, conv_tol: float = 1.0e-8, replicas=None):
        """``TDVPEngine.operate`` for every selected replica in ONE launch and one host wait (``k_batch_operate``, one
        workgroup per selected replica): each replica's state becomes ``phi ~ O|psi> / |O|psi>|``, fitted in the bond
        dimensions of ``psi`` by up to ``maxstep`` double sweeps, ``O`` the MPO the replica carries under ``op_id``
        (``set_mpo``, its ``shift`` included); a replica stops on its own when ``|1 - |<phi_i|phi_{i-1}>|| < conv_tol``.
        The fit is exact only where ``O psi`` fits the bonds.  ``replicas``: a list of distinct replica indices, default
        all.  The selected replicas must have their centre at site 0 and are left normalised, centre at site 0.

        Returns ``{"norms": (B,), "iterations": (B,) int, "statuses": list}`` indexed by replica: the norm ``|O psi|``
        of the last apply and the double sweeps run; entries of replicas that were not selected are 0.  A replica that
        the operator annihilates stops with norm 0 while the others finish; the call then raises that replica's error
        and leaves every status in ``statuses``, as ``propagate`` does, and the norms and counts in ``operated``."""
        n = len(self.engines)
        op_id, maxstep, conv_tol, sel = operate_request(n, op_id, maxstep, conv_tol, replicas)
        norms = np.zeros(n, dtype=np.float64)
        iters = np.zeros(n, dtype=np.int32)
        rep = None if sel is None else (C.c_int * len(sel))(*sel)
        nsel = 0 if sel is None else len(sel)
        self.operated = {"norms": norms, "iterations": iters}  # what the call filled in is kept when it raises
        self._run(lambda b, st: self._lib.mitdvp_batch_operate(b, op_id, maxstep, conv_tol, rep, nsel, _dp(norms),
                                                                iters.ctypes.data_as(C.POINTER(C.c_int)), st))
        return {"norms": norms, "iterations": iters, "statuses": list(self.statuses)}

    # ---- ground states by improved relaxation (mitdvp_batch_relax) ----
    def relax(self, maxstep: int = 20, conv_tol: float = 0.0):
        """Up to ``maxstep`` improved-relaxation steps of every replica in ONE launch and one host wait
        (``k_batch_relax``); the replicas must have been made with ``relax="improved"`` and have their centre at site 0.
        ``E_n``, a replica's energy after step ``n``, is the lowest Ritz value of its last local solve.  With
        ``conv_tol > 0`` a replica stops on its own once ``|E_n - E_{n-1}| <= conv_tol`` while the others go on;
        ``conv_tol = 0`` runs ``maxstep`` steps.

        Returns ``{"energy": (B,), "steps": (B,) int, "history": (B, maxstep)}``: the last ``E_n``, the steps run, and
        ``E_1 .. E_n`` of each replica with NaN behind its stop.  A replica whose local solve does not converge in
        ``max_diag_krylov`` vectors stops while the others finish; the call then raises that replica's error and leaves
        every status in ``statuses`` and what was filled in in ``relaxed``, as ``propagate`` does."""
        n = len(self.engines)
        maxstep = int(maxstep)
        conv_tol = float(conv_tol)
        if maxstep < 1:
            raise ValueError(f"relax: maxstep = {maxstep}, it must be >= 1")
        if not (conv_tol >= 0.0) or not np.isfinite(conv_tol):
            raise ValueError(f"relax: conv_tol = {conv_tol}, it must be finite and >= 0")
        energy = np.full(n, np.nan, dtype=np.float64)
        steps = np.zeros(n, dtype=np.int32)
        history = np.full((n, maxstep), np.nan, dtype=np.float64)
        self.relaxed = {"energy": energy, "steps": steps, "history": history}
        self._run(lambda b, st: self._lib.mitdvp_batch_relax(b, maxstep, conv_tol, _dp(energy),
                                                              steps.ctypes.data_as(C.POINTER(C.c_int)), _dp(history), st))
        return dict(self.relaxed)

    # ---- excited states by deflation against stored states (mitdvp_batch_deflate_*) ----
    def deflate_push(self, weights):
        """Stores the present state of every replica in the next free slot of the batch's deflation set
        (``mitdvp_batch_deflate_push``; at most 8 slots, ONE launch).  ``weights``: a scalar, or one weight per replica,
        finite and ``> 0``.  The replicas must be ``relax="improved"`` ones with their centre at site 0, as ``relax``
        leaves them, and normalised.  While the set is not empty ``relax`` (and ``propagate`` / ``sweep``) solve every
        local problem on ``H_eff + sum_k w_k |q_k><q_k|`` with ``q_k`` the stored state ``k`` in the replica's site basis
        (``k_batch_relax_defl``): from a fresh start the replicas then relax to the lowest state orthogonal to the stored
        ones, provided every weight exceeds the gap to it.  ``relax``'s ``"energy"`` is then the energy plus
        ``sum_k w_k |<phi_k|psi>|^2``; ``propagate(0, 0, observe={"energy": True})`` gives ``<psi|H|psi>``.  The library
        validates and names what it refuses; a refused call changes nothing."""
        n = len(self.engines)
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(weights, dtype=np.float64), (n,)) if np.ndim(weights) == 0
                                 else np.asarray(weights, dtype=np.float64))
        if w.shape != (n,):
            raise ValueError(f"deflate_push: {w.shape} weights for {n} replicas (a scalar, or one weight per replica)")
        _lib.check(self._lib.mitdvp_batch_deflate_push(self._handle(), _dp(w)))

    def deflate_clear(self):
        """Empties the deflation set (``mitdvp_batch_deflate_clear``): ``relax`` finds ground states again, bit for bit."""
        _lib.check(self._lib.mitdvp_batch_deflate_clear(self._handle()))

    def deflate_count(self) -> int:
        """The number of stored states (``mitdvp_batch_deflate_count``)."""
        c = C.c_int(0)
        _lib.check(self._lib.mitdvp_batch_deflate_count(self._handle(), C.byref(c)))
        return int(c.value)

    def deflate_overlaps(self):
        """``(count, B)`` complex: ``<phi_k|psi_r>`` of every stored state ``k`` with replica ``r`` as it is now, ONE launch
        (``mitdvp_batch_deflate_overlaps``); nothing is written to the replicas or the slots."""
        n = len(self.engines)
        k = self.deflate_count()
        out = np.zeros((k, n, 2), dtype=np.float64)
        if k:
            _lib.check(self._lib.mitdvp_batch_deflate_overlaps(self._handle(), _dp(out)))
        return out[..., 0] + 1j * out[..., 1]

    def launches(self) -> int:
        """kernel launches counted so far on replica 0, where the batch's launches are counted once"""
        return int(self.engines[0].counters()["n_launch"])

    def set_relax_restarts(self, n: int):
        """Lets a local Lanczos solve of ``relax="improved"`` replicas restart up to ``n`` times
        (``mitdvp_batch_set_relax_restarts``): a solve that has not converged after ``max_diag_krylov`` (at most 64)
        vectors keeps its lowest Ritz vector and the next Lanczos vector and goes on, at no further apply and no further
        memory, so that hard realisations converge and a small ``max_diag_krylov`` becomes usable.  ``n = 0``, the default
        of a batch, is the solve without restarts, bit for bit; ``n`` is at most 4096.  The setting holds for ``relax``,
        ``propagate`` and ``sweep`` alike, and the call clears the counters of ``relax_restarts``.  The library validates
        (the replicas' ``relax``, the range) and a refused call leaves the setting before in place."""
        n = int(n)
        _lib.check(self._lib.mitdvp_batch_set_relax_restarts(self._handle(), n))
        self._restarts = n

    def relax_restarts(self):
        """``{"total": (B,) int64, "most": (B,) int32}``: the restarts every replica has taken since
        ``set_relax_restarts`` (or since the batch was made), and the most restarts of any one of its local solves."""
        n = len(self.engines)
        total = np.zeros(n, dtype=np.int64)
        most = np.zeros(n, dtype=np.int32)
        _lib.check(self._lib.mitdvp_batch_relax_restarts(self._handle(), total.ctypes.data_as(C.POINTER(C.c_longlong)),
                                                         most.ctypes.data_as(C.POINTER(C.c_int))))
        return {"total": total, "most": most}

    def _run(self, call):
        n = len(self.engines)
        st = (C.c_int * n)()
        rc = call(self._handle(), st)
        self.statuses = list(st)
        if rc != 0:
            bad = next((i for i in range(n) if st[i] != 0), None)
            if bad is None:
                _lib.check(rc)  # the call itself was refused
            _lib.check(st[bad], self.engines[bad]._h)

    def propagate(self, dt_au: float, nsteps: int = 1, observe: dict | None = None, every: int = 1):
        """``nsteps`` time steps of every replica: two launches per time step for the whole batch.

        ``observe=None``: nothing else, returns ``None``.  ``observe=dict(...)`` with the arguments of ``observe``: a
        recorded run (``mitdvp_batch_run``) -- the state before step 0 and after every ``every``-th step is observed on
        the device, one launch per record, and everything comes back at the end of the call; returns what ``observe``
        returns with a leading record axis of ``nsteps // every + 1``.  ``observe`` may also carry ``keys=[...]``, keys as
        ``densities`` takes them: they are recorded in the same run by one more launch per record (``k_batch_density``) and
        come back as ``mean_density`` / ``density``, record axis first; the other entries are bitwise what they are
        without ``keys``.  ``cross=True`` adds the request of ``set_cross``, which every record of a run evaluates while
        it is set (one more launch per record): ``cross`` of shape ``(nrec, P)`` and ``mean_cross`` ``(nrec,)``, the
        weighted sum over the pairs with ``cross_weights`` (P numbers, default 1 / P each).  ``spectra=True`` adds the
        request of ``set_spectra`` in the same way (``k_batch_spectra``, one more launch per record): the entries of
        ``spectra()`` with a leading record axis, averaged with ``spectra_weights`` (B numbers, default 1 / B each).  With
        ``norm=True`` the entry ``mean_norm2`` stays the observation's ``(nrec,)`` array, which every bond's sum of
        weights equals.  ``samples=True`` adds the request of ``set_samples`` (``k_batch_sample``, one more launch per
        record; a record draws with the batch's step counter as it stands at that record): the entries of ``samples()``
        with a leading record axis, ``mean_freq`` formed with ``samples_weights`` (B numbers, default 1 / B each).
        ``expect=True`` adds the request of ``set_expect`` (``k_batch_expect``, one more launch per record): ``expect`` of
        shape ``(nrec, B, nops)`` and ``mean_expect`` ``(nrec, nops)``, averaged with ``expect_weights`` (B numbers,
        default 1 / B each).  ``cross_mpo=True`` adds the request of ``set_cross_mpo`` (``k_batch_cross_mpo``, one more launch
        per record): ``cross_mpo`` of shape ``(nrec, P)`` and ``mean_cross_mpo`` ``(nrec,)``, the weighted sum over the entries
        with ``cross_mpo_weights`` (P numbers, default 1 / P each)."""
        if observe is None:
            self._run(lambda b, st: self._lib.mitdvp_batch_step(b, float(dt_au), int(nsteps), st))
            return None
        return self._observed(float(dt_au), int(nsteps), int(every), **observe)

    def observe(self, sites=(), norm: bool = True, autocorr: bool = False, energy: bool = False, weights=None,
                per_replica: bool = True):
        """The current state of every replica observed by ONE launch, the ensemble means formed by a second one
        (``mitdvp_batch_observe``); all replicas must have their centre at site 0.  ``sites``: strictly ascending sites
        whose one-site reduced densities are wanted.  Returns a dict of NumPy arrays: ``mean_norm2`` (the mean of the
        SQUARED norms), ``mean_autocorr``, ``mean_energy``, ``mean_rdm`` (a list of (d, d) arrays, one per site) and, with
        ``per_replica``, ``norm`` (B,), ``autocorr`` (B,), ``energy`` (B,), ``rdm`` (a list of (B, d, d) arrays) -- only
        what was asked.  ``weights``: B numbers, default 1 / B each."""
        rec = self._observed(0.0, 0, 1, sites=sites, norm=norm, autocorr=autocorr, energy=energy, weights=weights,
                             per_replica=per_replica)
        return {k: ([x[0] for x in v] if isinstance(v, list) else v[0]) for k, v in rec.items()}

    def densities(self, keys, weights=None, per_replica: bool = True):
        """Multi-site reduced densities of the current state of every replica by ONE launch (``k_batch_density``), their
        ensemble means by a second one (``mitdvp_batch_observe_keys``); all replicas must have their centre at site 0.
        ``keys``: a list of keys in the reference's form, a tuple of site indices, non-decreasing, each site once (its
        diagonal) or twice (ket and bra): ``(0, 0, 2, 2)``, ``(0, 1)``, ``(1, 2, 2)``.  Returns a dict: ``mean_density``,
        a list with one array per key shaped like ``TDVPEngine.reduced_density(legs)``, and, with ``per_replica``,
        ``density``, a list of ``(B, ...)`` arrays.  A malformed key is a ``ValueError`` naming it, raised before the GPU
        is touched.  ``weights``: B numbers, default 1 / B each."""
        keys = list(keys)
        if not keys:
            raise ValueError("densities: no key")
        rec = self._observed(0.0, 0, 1, norm=False, weights=weights, per_replica=per_replica, keys=keys)
        return {k: [x[0] for x in v] for k, v in rec.items()}

    def _observed(self, dt_au, nsteps, every, sites=(), norm=True, autocorr=False, energy=False, weights=None, per_replica=True,
                  keys=(), cross=False, cross_weights=None, spectra=False, spectra_weights=None, samples=False,
                  samples_weights=None, expect=False, expect_weights=None, cross_mpo=False, cross_mpo_weights=None):
        n = len(self.engines)
        if cross:
            # no request, or weights of the wrong length: raised before any library call
            self._request_weights("cross", "pair", cross_weights)
        if spectra:
            self._request_weights("spectra", "replica", spectra_weights)
        if samples:
            self._request_weights("samples", "replica", samples_weights)
        if expect:
            self._request_weights("expect", "replica", expect_weights)
        if cross_mpo:
            self._request_weights("cross_mpo", "entry", cross_mpo_weights)
        nsite = self.engines[0].nsite
        legs = [density_key_legs(k, nsite) for k in keys]  # a malformed key raises here, before any library call
        sites = [int(p) for p in sites]
        what = ((_lib.OBS_NORM if norm else 0) | (_lib.OBS_AUTOCORR if autocorr else 0) | (_lib.OBS_ENERGY if energy else 0)
                | (_lib.OBS_RDM if sites else 0))
        w = None
        if weights is not None:
            w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
            if w.shape != (n,):
                raise ValueError(f"weights must be {n} numbers, one per replica (got shape {w.shape})")
        b = self._handle()
        sarr = (C.c_int * max(len(sites), 1))(*sites)
        cnt = (C.c_size_t * 4)()
        wp = None if w is None else _dp(w)
        larr = (C.c_int * max(len(legs) * nsite, 1))(*[x for row in legs for x in row])
        dens = {"density": None, "mean_density": None}

        def call(bb, outp, st):  # without keys: the entry point of before
            if not legs:
                return self._lib.mitdvp_batch_run(bb, dt_au, nsteps, every, sarr, len(sites), what, wp, outp, cnt, st)
            dp = [None if a is None else _dp(a) for a in (dens["density"], dens["mean_density"])]
            return self._lib.mitdvp_batch_run_keys(bb, dt_au, nsteps, every, sarr, len(sites), larr, len(legs), what, wp, outp,
                                                   dp[0], dp[1], cnt, st)

        _lib.check(call(b, None, None))
        nrec, _, nrdm, ndens = (int(c) for c in cnt)
        out = _lib.BatchOut()
        keep = {}

        def want(name, shape, dtype):
            keep[name] = np.zeros(shape, dtype=dtype)
            setattr(out, name, _dp(keep[name]))

        if norm:
            want("mean_norm2", (nrec,), np.float64)
        if autocorr:
            want("mean_autocorr", (nrec,), np.complex128)
        if energy:
            want("mean_energy", (nrec,), np.complex128)
        if sites:
            want("mean_rdm", (nrec, nrdm), np.complex128)
        if per_replica:
            if norm:
                want("norm", (nrec, n), np.float64)
            if autocorr:
                want("autocorr", (nrec, n), np.complex128)
            if energy:
                want("energy", (nrec, n), np.complex128)
            if sites:
                want("rdm", (nrec, n, nrdm), np.complex128)
        if legs:
            dens["mean_density"] = keep["mean_density"] = np.zeros((nrec, ndens), dtype=np.complex128)
            if per_replica:
                dens["density"] = keep["density"] = np.zeros((nrec, n, ndens), dtype=np.complex128)
        try:
            self._run(lambda bb, st: call(bb, C.byref(out), st))
        finally:
            self.records = self._split(keep, sites, legs)  # a replica that did not converge raises; what was recorded stays readable here
            if cross:
                self.records["cross"], self.records["mean_cross"] = self._cross_records(cross_weights)
            if spectra:
                for k, v in self._spectra_records(spectra_weights, per_replica).items():
                    self.records.setdefault(k, v)  # norm=True owns mean_norm2: every bond's W is that very number
            if samples:
                self.records.update(self._samples_records(samples_weights, per_replica))
            if expect:
                self.records.update(self._expect_records(expect_weights, per_replica))
            if cross_mpo:
                self.records["cross_mpo"], self.records["mean_cross_mpo"] = self._cross_mpo_records(cross_mpo_weights)
        return self.records

    def _split(self, keep, sites, legs=()):
        """the flat RDM axis cut into one (.., d, d) array per observed site, the flat density axis into one array per key"""
        res = dict(keep)
        alld = [self.engines[0].get_site_shape(p)[1] for p in range(self.engines[0].nsite)] if legs else []
        for name in ("mean_density", "density"):
            if name in res:
                flat, parts, at = res[name], [], 0
                for row in legs:
                    shape = tuple(alld[p] for p, k in enumerate(row) for _ in range(k))
                    size = int(np.prod(shape))
                    parts.append(flat[..., at:at + size].reshape(flat.shape[:-1] + shape))
                    at += size
                res[name] = parts
        dims = [self.engines[0].get_site_shape(p)[1] for p in sites]
        for name in ("mean_rdm", "rdm"):
            if name in res:
                flat, parts, at = res[name], [], 0
                for d in dims:
                    parts.append(flat[..., at:at + d * d].reshape(flat.shape[:-1] + (d, d)))
                    at += d * d
                res[name] = parts
        return res

    def sweep(self, dt_au: float, forward: bool):
        self._run(lambda b, st: self._lib.mitdvp_batch_sweep(b, float(dt_au), int(bool(forward)), st))

    def _drop(self):
        if getattr(self, "_b", None) is not None:
            self._lib.mitdvp_batch_destroy(self._b)
            self._b = None

    def close(self):
        self._drop()
        if self._own:
            for e in self.engines:
                e.close()
        self.engines = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_cu_count(device: int = 0) -> int:
    """compute units of the device (256 on MI355X)"""
    n = C.c_int()
    _lib.check(_lib.load().mitdvp_device_cu_count(device, C.byref(n)))
    return n.value


def set_gemm_mode(mode: str):
    """"4m" (textbook complex product) or "3m" (Karatsuba, library default)."""
    _lib.load().mitdvp_set_gemm_mode({"4m": 0, "3m": 1}[mode.lower()])


def set_qr_fast(on: bool):
    """QR panels by CholeskyQR2 + Householder reconstruction (True, library default) or one Householder step per
    launch only (False); process-wide."""
    _lib.load().mitdvp_set_qr_fast(int(bool(on)))


def bench_qr(m: int, n: int, reps: int = 10, device: int = 0):
    """(milliseconds, launches) per m x n QR gauge move on the device (HIP events around `reps` factorisations)."""
    ms, nl = C.c_double(), C.c_long()
    _lib.check(_lib.load().mitdvp_bench_qr(device, m, n, reps, C.byref(ms), C.byref(nl)))
    return ms.value, nl.value


def qr_thin(a=None, shape=None, gauge_free: bool = True, reps: int = 1, device: int = 0):
    """The thin QR of the sweep's gauge moves (``mitdvp_qr_thin``): ``a`` (m x n) or, with ``shape=(m, n)``, a random
    matrix generated on the device.  Returns (Q, R, info) with info = {"ms", "launches", "gauge_free_path"}; Q, R are None
    for a device-generated input."""
    if a is not None:
        a = _c128(a)
        m, n = a.shape
        q, r = np.empty((m, n), dtype=np.complex128), np.empty((n, n), dtype=np.complex128)
    else:
        m, n = shape
        q = r = None
    ms, nl, path = C.c_double(), C.c_long(), C.c_int()
    _lib.check(_lib.load().mitdvp_qr_thin(device, _dp(a) if a is not None else None, m, n, int(bool(gauge_free)),
                                          _dp(q) if q is not None else None, _dp(r) if r is not None else None, reps,
                                          C.byref(ms), C.byref(nl), C.byref(path)))
    return q, r, {"ms": ms.value, "launches": nl.value, "gauge_free_path": bool(path.value)}


def get_qr_fast() -> bool:
    return bool(_lib.load().mitdvp_get_qr_fast())


def device_count() -> int:
    """HIP devices visible to this process (0 on a CPU-only box); does not create a context."""
    n = C.c_int()
    _lib.check(_lib.load().mitdvp_device_count(C.byref(n)))
    return n.value


def device_sync(device: int = 0) -> None:
    _lib.check(_lib.load().mitdvp_device_sync(device))


def get_gemm_mode() -> str:
    return "3m" if _lib.load().mitdvp_get_gemm_mode() else "4m"


def bench_heff(dl, d, dr, ml, mr, reps=3, warmup=1, device=0) -> float:
    ms = C.c_double()
    _lib.check(_lib.load().mitdvp_bench_heff(device, dl, d, dr, ml, mr, reps, warmup, C.byref(ms)))
    return ms.value


def mfma_peak_probe(device=0) -> float:
    out = C.c_double()
    _lib.check(_lib.load().mitdvp_mfma_peak_probe(device, C.byref(out)))
    return out.value


def mfma_layout_probe(device=0) -> np.ndarray:
    out = (C.c_int * 512)()
    _lib.check(_lib.load().mitdvp_mfma_layout_probe(device, out))
    return np.array(out).reshape(64, 4, 2)
