"""Context: thin object wrapper over the fine-grained C ABI (hb_ctx_*), used by bench.py and by
the kernel-level parity tests. Everything computes on the device; see include/hibayes_gpu.h."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import CtxParams, LaunchStats, SweepIn, SweepOut, SweepTiming, HB_MAX_FOLD, HB_ND, check, lib

MODEL_INDEX = {"BayesRR": 1, "BayesA": 2, "BayesB": 3, "BayesBpi": 3, "BayesC": 4, "BayesCpi": 4,
               "BayesL": 5, "BayesR": 6}


def live_buffers():
    """(buffers, bytes): the device and pinned buffers the library holds in this process right now, over every context, run and handle
    (hb_debug_live_buffers). Back at its earlier value after every close(), destroy and free."""
    nb, by = C.c_int64(), C.c_int64()
    check(lib().hb_debug_live_buffers(C.byref(nb), C.byref(by)))
    return nb.value, by.value


class Context:
    def __init__(self, n, m, device=0, panel=0, precise=2, m_offset=0, seed=666666):
        self.L = lib()
        p = CtxParams(device=device, n=n, m=m, panel=panel, precise=int(precise), m_offset=m_offset, seed=seed)
        h = C.c_void_p()
        check(self.L.hb_ctx_create(C.byref(p), C.byref(h)))
        self.h, self.n, self.m, self.device = h, n, m, device

    def close(self):
        if self.h:
            self.L.hb_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def panel(self):
        return self.L.hb_ctx_panel(self.h)

    @property
    def ld(self):
        return self.L.hb_ctx_ld(self.h)

    # ---- genotypes ----
    def upload(self, X, col0=0):
        X = np.asarray(X)
        if X.dtype == np.int8:
            Xa = np.asfortranarray(X)
            # (the stride numpy reports for a single column is arbitrary: at least a column's length)
            check(self.L.hb_ctx_upload_genotype_i8(self.h, Xa.ctypes.data, max(Xa.strides[1], Xa.shape[0]), col0, Xa.shape[1]))
        else:
            Xa = np.asfortranarray(X, dtype=np.float64)
            check(self.L.hb_ctx_upload_genotype_f64(self.h, Xa.ctypes.data, max(Xa.strides[1] // 8, Xa.shape[0]), col0, Xa.shape[1]))

    def upload_real(self, X):
        """Real-valued genotypes (imputed dosages), n x m: any finite value as it is, into the fp64 resident layout (genotype_bits = 64). The
        context then sweeps on the per-panel kernels (pipeline_note() says so); a NaN or Inf raises with status 1."""
        Xa = np.asfortranarray(X, dtype=np.float64)
        if Xa.ndim != 2 or Xa.shape != (self.n, self.m):
            raise ValueError("upload_real: X must be %d x %d" % (self.n, self.m))
        check(self.L.hb_ctx_upload_genotype_real(self.h, Xa.ctypes.data, max(Xa.strides[1] // 8, Xa.shape[0])))

    def download_real(self):
        """The fp64 resident layout's columns, bit for bit what upload_real() was given."""
        out = np.zeros((self.n, self.m), dtype=np.float64, order="F")
        check(self.L.hb_ctx_download_genotype_real(self.h, out.ctypes.data, self.n))
        return out

    def upload_bed(self, raw, nind, rows=None, col0=0, ncols=None):
        raw = np.frombuffer(raw, dtype=np.uint8)
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        check(self.L.hb_ctx_upload_bed(self.h, raw.ctypes.data, raw.size, nind, None if r is None else r.ctypes.data,
                                       col0, self.m if ncols is None else ncols))

    def generate(self, seed, mono_every=0):
        check(self.L.hb_ctx_generate_genotype(self.h, seed, mono_every))

    def download(self, col0=0, ncols=None):
        ncols = self.m - col0 if ncols is None else ncols
        out = np.zeros((self.n, ncols), dtype=np.int8, order="F")
        check(self.L.hb_ctx_download_genotype(self.h, out.ctypes.data, self.n, col0, ncols))
        return out

    def marker_stats(self):
        xpx, vx = np.zeros(self.m), np.zeros(self.m)
        s, z = C.c_double(), C.c_int32()
        check(self.L.hb_ctx_marker_stats(self.h, xpx.ctypes.data, vx.ctypes.data, C.byref(s), C.byref(z)))
        return xpx, vx, s.value, z.value

    def set_layout(self, bits=2, keep_int8=True):
        """Resident genotype layout the sweep reads: 8 (int8 columns) or 2 (2 bits per genotype, a quarter of the bytes); 64 converts the
        int8 columns to the fp64 layout of upload_real()."""
        check(self.L.hb_ctx_set_layout(self.h, int(bits), 1 if keep_int8 else 0))

    def layout(self):
        b, k = C.c_int32(), C.c_int32()
        check(self.L.hb_ctx_get_layout(self.h, C.byref(b), C.byref(k)))
        return b.value, bool(k.value)

    def set_adaptive(self, on=True):
        """Let Bayes() choose the geometry of each sweep of a point-mass model from the number of moves of the previous one."""
        check(self.L.hb_ctx_set_adaptive(self.h, 1 if on else 0))

    def set_pipeline(self, pipeline=1, lookahead=2, dotgroup=4):
        check(self.L.hb_ctx_set_pipeline(self.h, pipeline, lookahead, dotgroup))

    def set_matvec_kernel(self, kind):
        """2-bit resident genotypes: 0 = k_dotq2 (v_dot4, default), 1 = k_dotq2r, 2 = k_dotq2m (matrix cores; an A/B). Same integers."""
        check(self.L.hb_ctx_set_matvec_kernel(self.h, kind))

    def debug_inject_abort(self, panel, times=1):
        """Debug hook: abort the next `times` pipeline sweeps once the chain has published `panel` panels (hb_run_step replays them)."""
        check(self.L.hb_ctx_debug_inject_abort(self.h, panel, times))

    def pre(self):
        """Debug read-out: (thr, invv, sdz) as k_pre left them in the last sweep, each kpad x m_pad (m_pad = whole panels)."""
        m_pad = -(-self.m // self.panel) * self.panel
        out = [np.zeros((7, m_pad)) for _ in range(3)]
        kp = C.c_int32()
        check(self.L.hb_ctx_debug_get_pre(self.h, C.byref(kp), *[x.ctypes.data for x in out]))
        return tuple(x[:kp.value].copy() for x in out)

    def mirrors(self):
        """Debug read-out: the residual version the last executed update rows wrote and its mirrors, as a dict — slot, bound_index (h of
        the bound mb[1 + h] behind the exponent; -1 before the first sweep), r (ld doubles, rows [n, ld) included), r32 (ld floats), rq (the
        HB_ND x ld int8 digit planes) and vexp (both None unless precise = 2), mb (the npanels + 2 bounds on max |yadj|)."""
        ld = self.ld
        npan = (self.m + self.panel - 1) // self.panel
        r, r32 = np.zeros(ld), np.zeros(ld, dtype=np.float32)
        rq, mb = np.zeros((HB_ND, ld), dtype=np.int8), np.zeros(npan + 2)
        slot, h, nd, ve = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(self.L.hb_ctx_debug_get_mirrors(self.h, C.byref(slot), C.byref(h), r.ctypes.data, r32.ctypes.data, C.byref(nd),
                                              rq.ctypes.data, C.byref(ve), mb.ctypes.data))
        if nd.value not in (0, HB_ND):
            raise RuntimeError("hb_ctx_debug_get_mirrors: %d digit planes, this binding knows %d" % (nd.value, HB_ND))
        return {"slot": slot.value, "bound_index": h.value, "r": r, "r32": r32, "rq": rq if nd.value else None,
                "vexp": ve.value if nd.value else None, "mb": mb}

    def cert(self):
        """Debug read-out: the group chain's certificate as build_gram() left it, as a dict — ok (False: there is none, the arrays are None), Lg
        (the band it was built over), ga, gB, gcmax (m_pad int32 each: G[k][j] = ga[k] gB[j] + c[k][j], |c[k][j]| <= gcmax[k])."""
        m_pad = -(-self.m // self.panel) * self.panel
        a = [np.zeros(m_pad, dtype=np.int32) for _ in range(3)]
        ok, lg = C.c_int32(), C.c_int32()
        check(self.L.hb_ctx_debug_get_cert(self.h, C.byref(ok), C.byref(lg), *[x.ctypes.data for x in a]))
        ga, gB, gcmax = a if ok.value else (None, None, None)
        return {"ok": bool(ok.value), "Lg": lg.value, "ga": ga, "gB": gB, "gcmax": gcmax}

    def opening(self):
        """Debug read-out: what k_hotlist wrote for the chain of the last pipelined sweep, as a dict — nslot, kappa, candf, thr0f (m_pad
        floats), opn (m_pad x 4 int32 records, None where none were written), slot_of (m_pad int32) and hotpack (npanels x 256 int32)."""
        P = self.panel
        npan = -(-self.m // P)
        thr0f, opn = np.zeros(npan * P, dtype=np.float32), np.zeros((npan * P, 4), dtype=np.int32)
        slot_of, hotpack = np.zeros(npan * P, dtype=np.int32), np.zeros((npan, 256), dtype=np.int32)
        ns, has, ka, cf = C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
        check(self.L.hb_ctx_debug_get_opening(self.h, C.byref(ns), C.byref(ka), C.byref(cf), C.byref(has), thr0f.ctypes.data, opn.ctypes.data,
                                              slot_of.ctypes.data, hotpack.ctypes.data))
        return {"nslot": ns.value, "kappa": ka.value, "candf": cf.value, "thr0f": thr0f, "opn": opn if has.value else None,
                "slot_of": slot_of, "hotpack": hotpack}

    def build_gram(self):
        s = C.c_double()
        check(self.L.hb_ctx_build_gram(self.h, C.byref(s)))
        return s.value

    def gram(self, p):
        P = self.panel
        G = np.zeros((P, P), dtype=np.int32)
        check(self.L.hb_ctx_download_gram(self.h, p, G.ctypes.data))
        return G

    def gram_real(self, p):
        """Panel p's Gram block on the fp64 resident layout (P x P doubles; hb_ctx_download_gram_real)."""
        P = self.panel
        G = np.zeros((P, P), dtype=np.float64)
        check(self.L.hb_ctx_download_gram_real(self.h, p, G.ctypes.data))
        return G

    def ldmat(self, chr=None, chisq=None, strip_bytes=0):
        """The LD variance-covariance matrix of the resident genotypes as an LDMatrix (hb_ldm_build; ldmat() of the reference,
        R/ldm.r:88-91): chr = m chromosome ids for one block per chromosome or None for the genome-wide matrix, chisq = None or the
        sparsification threshold. hibayes_amd.ldmat() is the full mirror with the reference's argument handling."""
        from .ldm import LDMatrix
        ch = None if chr is None else np.ascontiguousarray(chr, dtype=np.int32)
        if ch is not None and ch.shape != (self.m,):
            raise ValueError("chr must hold one chromosome id per marker")
        h = C.c_void_p()
        check(self.L.hb_ldm_build(self.h, None if ch is None else ch.ctypes.data, 0 if chisq is None else 1,
                                  0.0 if chisq is None else float(chisq), int(strip_bytes), C.byref(h)))
        return LDMatrix(h, self.device)

    def pipeline_note(self):
        v = self.L.hb_ctx_pipeline_note(self.h)
        return None if v is None else v.decode()

    def matmul(self, A):
        """X @ A on the device (A: m x R); the GEBV sample matrix of R/bayes.r:303-305."""
        A = np.asfortranarray(A, dtype=np.float64).reshape(self.m, -1, order="F")
        out = np.zeros((self.n, A.shape[1]), order="F")
        check(self.L.hb_ctx_matmul(self.h, A.ctypes.data, self.m, A.shape[1], out.ctypes.data, self.n))
        return out

    def window_var(self, A, windindx, nw=None):
        """(var, total): var[w - 1, r] = var(X_w alpha_w,r) over the individuals for every window id w of windindx (m ids in 1 .. nw) and every
        record r (column of A, m x R), total[r] = var(X alpha_r); N - 1 denominators. On the device from the resident genotypes
        (hb_ctx_window_var); hibayes_amd.window_pve() makes PVE and WPPA of them. nw: the number of windows where it is more than the largest id used
        (the rows past it, like every window without an effect, are 0.0)."""
        A = np.asfortranarray(A, dtype=np.float64).reshape(self.m, -1, order="F")
        wi = np.asarray(windindx)
        if wi.shape != (self.m,) or wi.dtype.kind not in "iu":
            raise ValueError("windindx must hold one integer window id per marker")
        if wi.min() < 1:
            raise ValueError("windindx must hold window ids in 1 .. nw")
        nw = int(wi.max()) if nw is None else int(nw)
        if nw < wi.max():
            raise ValueError("windindx must hold window ids in 1 .. nw")
        wi = np.ascontiguousarray(wi, dtype=np.uint32)
        var, total = np.zeros((nw, A.shape[1]), order="F"), np.zeros(A.shape[1])
        check(self.L.hb_ctx_window_var(self.h, A.ctypes.data, self.m, A.shape[1], wi.ctypes.data, nw, var.ctypes.data, nw, total.ctypes.data))
        return var, total

    def gram_band(self, p, l):
        P = self.panel
        G = np.zeros((P, P), dtype=np.int32)
        check(self.L.hb_ctx_download_gram_band(self.h, p, l, G.ctypes.data))
        return G

    def pipeline(self):
        v = [C.c_int32() for _ in range(4)]
        check(self.L.hb_ctx_get_pipeline(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)   # (pipeline, lookahead groups, panels per mat-vec, band blocks)

    def events(self):
        """Move lists of the last sweep as [(panel-local marker indices, deltas)] per panel."""
        P = self.panel
        npan = (self.m + P - 1) // P
        cnt = np.zeros(npan, dtype=np.int32)
        idx = np.zeros(npan * P, dtype=np.int32)
        dl = np.zeros(npan * P)
        check(self.L.hb_ctx_get_events(self.h, cnt.ctypes.data, idx.ctypes.data, dl.ctypes.data))
        return cnt, [(idx[p * P:p * P + cnt[p]].copy(), dl[p * P:p * P + cnt[p]].copy()) for p in range(npan)]

    # ---- state ----
    def set_residual(self, yadj=None, u=None):
        a = None if yadj is None else np.ascontiguousarray(yadj, dtype=np.float64)
        b = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
        check(self.L.hb_ctx_set_residual(self.h, None if a is None else a.ctypes.data, None if b is None else b.ctypes.data))

    def get_residual(self):
        r, u = np.zeros(self.n), np.zeros(self.n)
        check(self.L.hb_ctx_get_residual(self.h, r.ctypes.data, u.ctypes.data))
        return r, u

    def set_effects(self, g=None, tracker=None, vargL=None):
        ga = None if g is None else np.ascontiguousarray(g, dtype=np.float64)
        ta = None if tracker is None else np.ascontiguousarray(tracker, dtype=np.uint8)
        va = None if vargL is None else np.ascontiguousarray(vargL, dtype=np.float64)
        check(self.L.hb_ctx_set_effects(self.h, *(None if x is None else x.ctypes.data for x in (ga, ta, va))))

    def get_effects(self):
        g, t, v = np.zeros(self.m), np.zeros(self.m, dtype=np.uint8), np.zeros(self.m)
        check(self.L.hb_ctx_get_effects(self.h, g.ctypes.data, t.ctypes.data, v.ctypes.data))
        return g, t, v

    def dot(self, col0=0, ncols=None):
        ncols = self.m - col0 if ncols is None else ncols
        d = np.zeros(ncols)
        check(self.L.hb_ctx_dot(self.h, col0, ncols, d.ctypes.data))
        return d

    def residual_sums(self):
        a, b = C.c_double(), C.c_double()
        check(self.L.hb_ctx_residual_sums(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def residual_shift(self, a):
        check(self.L.hb_ctx_residual_shift(self.h, float(a)))

    def set_covariates(self, Cm):
        Cm = np.asfortranarray(Cm, dtype=np.float64).reshape(self.n, -1, order="F")
        check(self.L.hb_ctx_set_covariates(self.h, Cm.ctypes.data, Cm.shape[1]))

    def cov_dot(self, i):
        v = C.c_double()
        check(self.L.hb_ctx_cov_dot(self.h, i, C.byref(v)))
        return v.value

    def cov_axpy(self, i, a):
        check(self.L.hb_ctx_cov_axpy(self.h, i, float(a)))

    def set_levels(self, zid, nlev):
        z = np.asfortranarray(zid, dtype=np.int32).reshape(self.n, -1, order="F")
        nl = np.ascontiguousarray(nlev, dtype=np.int32)
        self._nlev = list(nl)
        check(self.L.hb_ctx_set_levels(self.h, z.ctypes.data, z.shape[1], nl.ctypes.data))

    def level_sums(self, t):
        s = np.zeros(self._nlev[t])
        check(self.L.hb_ctx_level_sums(self.h, t, s.ctypes.data))
        return s

    def level_axpy(self, t, delta):
        d = np.ascontiguousarray(delta, dtype=np.float64)
        check(self.L.hb_ctx_level_axpy(self.h, t, d.ctypes.data))

    def blocks_setup(self, cpc, zz, vrtmp0):
        """Device-resident covariate / random-effect state (reference src/Bayes.cpp:484-516); after set_covariates / set_levels."""
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (cpc, zz, vrtmp0)]
        self._blk = (len(a[0]), len(a[1]), len(a[2]))
        check(self.L.hb_ctx_blocks_setup(self.h, *[x.ctypes.data for x in a]))

    def blocks_step(self, vare, z_beta, z_levels, chisq, dfr, s2r):
        """Enqueue the iteration's covariate and random-effect kernels with the host's pre-drawn deviates (no host sync)."""
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (z_beta, z_levels, chisq)]
        check(self.L.hb_ctx_blocks_step(self.h, float(vare), *[x.ctypes.data for x in a], float(dfr), float(s2r)))

    def blocks_state(self):
        nc, nl, nr = self._blk
        out = [np.zeros(nc), np.zeros(nl), np.zeros(nr), np.zeros(nr)]
        check(self.L.hb_ctx_blocks_state(self.h, *[x.ctypes.data for x in out]))
        return out

    # ---- BSLMM's polygenic block (reference src/Bayes.cpp:518-552) ----
    def poly_setup(self, Kival, Ki, on_device=False):
        """Eigenvalues (n) and eigenvectors (n x n) of the relationship matrix. Ki: a host array, or with on_device=True a CUDA/HIP torch
        tensor (float64, row j = column j of K, an even row stride) that the context borrows and this object keeps alive; or an
        eig.EigVectors handle (make_grm(eigen_solver="device", keep_on_device=True)), borrowed and kept alive likewise."""
        kv = np.ascontiguousarray(Kival, dtype=np.float64)
        from .eig import EigVectors
        if isinstance(Ki, EigVectors):
            Ki._live("poly_setup")
            if Ki.n != self.n or kv.size != self.n:
                raise ValueError("poly_setup: the eigenvectors are %d x %d, the context holds %d individuals" % (Ki.n, Ki.n, self.n))
            self._poly_keep = Ki
            check(self.L.hb_ctx_poly_setup(self.h, kv.ctypes.data, Ki.ptr, Ki.ld, 1))
        elif on_device:
            if Ki is None or Ki.dim() != 2 or Ki.shape[0] != self.n or Ki.shape[1] < self.n or Ki.stride(1) != 1:
                raise ValueError("poly_setup: a device K is a tensor of n rows, row j holding column j of K (n values, then padding)")
            self._poly_keep = Ki
            check(self.L.hb_ctx_poly_setup(self.h, kv.ctypes.data, Ki.data_ptr(), Ki.stride(0), 1))
        else:
            K = np.asfortranarray(Ki, dtype=np.float64)
            check(self.L.hb_ctx_poly_setup(self.h, kv.ctypes.data, K.ctypes.data, K.strides[1] // 8, 0))

    def poly_step(self, vare, vb_in, seed, it, chis, s2_df):
        """Enqueue one iteration of the block (no host sync): vb_in < 0 keeps the device's vb."""
        check(self.L.hb_ctx_poly_step(self.h, float(vare), float(vb_in), int(seed), int(it), float(chis), float(s2_df)))

    def poly_state(self):
        """(k, vb, q, flag) after the last step; flag: the matrix failed the reference's positive-definiteness check (:533)."""
        k = np.zeros(self.n)
        vb, q, fl = C.c_double(), C.c_double(), C.c_int32()
        check(self.L.hb_ctx_poly_state(self.h, k.ctypes.data, C.byref(vb), C.byref(q), C.byref(fl)))
        return k, vb.value, q.value, bool(fl.value)

    def poly_debug(self):
        """Debug read-out of the last step: t = K'(yadj + k_old), w, eval, Kg = K' k_new."""
        out = [np.zeros(self.n) for _ in range(4)]
        check(self.L.hb_ctx_poly_debug_get(self.h, *[x.ctypes.data for x in out]))
        return dict(zip(("t", "w", "eval", "Kg"), out))

    # ---- the single-step model's epsilon block (reference src/Bayes.cpp:554-584) ----
    def epsl_setup(self, y_J, Gi, index):
        """y_J (n), Gi (q x q: a scipy sparse matrix or an (indptr, indices, data) CSC triple of the full symmetric matrix) and index (the
        1-based column of Gi of each of the LAST len(index) individuals). epsilon and J start at 0."""
        from .ssbayes import epsl_descriptor
        gi, idx, keep = epsl_descriptor(Gi, index)
        yj = np.ascontiguousarray(y_J, dtype=np.float64).ravel()
        if yj.size != self.n:
            raise ValueError("epsl_setup: y_J holds %d values, the context %d individuals" % (yj.size, self.n))
        d = _lib.EpslDesc(C.pointer(gi), idx.ctypes.data, yj.ctypes.data)
        check(self.L.hb_ctx_epsl_setup(self.h, C.byref(d)))
        self._epsl_q = gi.q
        del keep

    def epsl_step(self, vare, veps_in, seed, it, zJ, chis, s2_df):
        """Enqueue one iteration of the block (no host sync): veps_in < 0 keeps the device's veps."""
        check(self.L.hb_ctx_epsl_step(self.h, float(vare), float(veps_in), int(seed), int(it), float(zJ), float(chis), float(s2_df)))

    def epsl_state(self):
        """(epsilon, veps, q = x'Gx, J) after the last step."""
        x = np.zeros(self._epsl_q)
        ve, q, J = C.c_double(), C.c_double(), C.c_double()
        check(self.L.hb_ctx_epsl_state(self.h, x.ctypes.data, C.byref(ve), C.byref(q), C.byref(J)))
        return x, ve.value, q.value, J.value

    def epsl_debug(self):
        """Debug read-out of the last step: b, the epsilon it started from, the J draw's y_J . yadj, and the schedule's counts."""
        b, xo, rhs, cnt = np.zeros(self._epsl_q), np.zeros(self._epsl_q), np.zeros(1), np.zeros(4, dtype=np.int32)
        check(self.L.hb_ctx_epsl_debug_get(self.h, b.ctypes.data, xo.ctypes.data, rhs.ctypes.data, cnt.ctypes.data))
        return {"b": b, "x_old": xo, "rhs": float(rhs[0]), "steps": int(cnt[0]), "launches": int(cnt[1]), "levels": int(cnt[2]), "max_col": int(cnt[3])}

    def epsl_force(self, sched_mode=0, row_mode=0):
        """Debug setter: rebuild the schedule with every step in single-workgroup launches (sched_mode 1) or wide (2), every row on a lane
        (row_mode 1) or a wave (2); 0 = the plan's own choice. The chain must not change by a bit."""
        check(self.L.hb_ctx_epsl_debug_set(self.h, int(sched_mode), int(row_mode)))

    def grm(self, lambda_=0.0, raw=False):
        """The genomic relationship matrix of the resident int8 genotypes (hb_grm_build; make_grm() of the reference, src/rm.cpp:5-53)."""
        from .grm import grm_build
        return grm_build(self, lambda_, raw)

    def set_windows(self, windindx):
        w = np.ascontiguousarray(windindx, dtype=np.uint32)
        self._nw = int(w.max())
        check(self.L.hb_ctx_set_windows(self.h, w.ctypes.data, self._nw))

    def get_windows(self):
        w = np.zeros(self._nw)
        check(self.L.hb_ctx_get_windows(self.h, w.ctypes.data))
        return w

    def counters(self):
        a, b, c = np.zeros(self.m), np.zeros(self.m), np.zeros(self.m)
        check(self.L.hb_ctx_get_counters(self.h, a.ctypes.data, b.ctypes.data, c.ctypes.data))
        return a, b, c

    # ---- one marker sweep ----
    @staticmethod
    def _sweep_in(model, it, vare, varg=0.0, logpi=(0.0, 0.0), fold=(0.0, 0.0), vara_fold=None, s2varg_df=0.0,
                  dfvara=4.0, lam=0.0, lam2=0.0, count_pip=False, store=False):
        si = SweepIn()
        si.model_index = MODEL_INDEX[model] if isinstance(model, str) else int(model)
        si.n_fold = len(logpi)
        si.iter = it
        si.vare, si.varg, si.s2varg_df, si.dfvara = vare, varg, s2varg_df, dfvara
        for k in range(len(logpi)):
            si.logpi[k] = logpi[k]
            si.fold[k] = fold[k] if k < len(fold) else 0.0
            si.vara_fold[k] = (vara_fold[k] if vara_fold is not None else varg * si.fold[k])
        si.lambda_, si.lambda2 = lam, lam2
        si.count_pip, si.store = int(count_pip), int(store)
        return si

    @staticmethod
    def _sweep_out(so):
        return {"sum_g2": so.sum_g2, "class_count": np.array(so.class_count[:]), "sum_vargL": so.sum_vargL,
                "sum_r": so.sum_r, "sum_r2": so.sum_r2, "var_u": so.var_u, "n_events": so.n_events}

    def sweep(self, model, it, vare, *a, **kw):
        si, so = self._sweep_in(model, it, vare, *a, **kw), SweepOut()
        check(self.L.hb_ctx_sweep(self.h, C.byref(si), C.byref(so)))
        return self._sweep_out(so)

    def sweep_range(self, block, nblocks, model, it, vare, *a, **kw):
        """Enqueue block `block` of a sweep cut into `nblocks` ranges of whole mat-vec groups (hb_ctx_sweep_range; the arguments
        of sweep() behind the two). sweep_end() after the last block fetches the sums."""
        si = self._sweep_in(model, it, vare, *a, **kw)
        check(self.L.hb_ctx_sweep_range(self.h, C.byref(si), int(block), int(nblocks)))

    def sweep_end(self):
        so = SweepOut()
        check(self.L.hb_ctx_sweep_end(self.h, C.byref(so)))
        return self._sweep_out(so)

    def time_matvec(self, reps=3):
        ms, nl, nc = C.c_double(), C.c_int32(), C.c_int32()
        check(self.L.hb_ctx_time_matvec(self.h, reps, C.byref(ms), C.byref(nl), C.byref(nc)))
        return ms.value, nl.value, nc.value

    def time_stream_read(self, reps=3):
        """(ms per pass, bytes per pass) of a plain streaming read of the resident genotype buffer: the measured ceiling the
        mat-vec's achieved bandwidth is quoted against beside the nominal HBM peak."""
        ms, nb = C.c_double(), C.c_int64()
        check(self.L.hb_ctx_time_stream_read(self.h, reps, C.byref(ms), C.byref(nb)))
        return ms.value, nb.value

    def matvec_stamps(self):
        """In-situ statistics of the mat-vec launches of the last sweep (set_profiling(8) first); see hb_launch_stats."""
        st = LaunchStats()
        check(self.L.hb_ctx_matvec_stamps(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in LaunchStats._fields_}

    def set_profiling(self, on):
        check(self.L.hb_ctx_set_profiling(self.h, int(on)))

    def last_timing(self):
        t = SweepTiming()
        check(self.L.hb_ctx_last_timing(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in SweepTiming._fields_}
