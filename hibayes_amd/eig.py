"""eigh(): the symmetric eigen-decomposition make_grm(eigen=True) needs (reference src/rm.cpp:46-52, eigen_sym_dc -> LAPACK dsyevd) with
its two O(n^3) stages on the device (hb_eig_*, hibayes_amd/csrc/hb_eig.hip):

    hb_eig_reduce    dsytrd: Q' A Q = T, panel-blocked Householder reflectors        device
    dstemr           eigenvalues w and eigenvectors Z of T (scipy.linalg.eigh_tridiagonal)   host, O(n^2) work
    hb_eig_vectors   dormtr: K = Q Z by block reflectors                             device

With tridiagonal="device" the middle stage is the device's too — hb_eig_tridiagonal (hibayes_amd/csrc/hb_stedc.hip): dstedc, Cuppen's divide and
conquer with Gu-Eisenstat vectors — and hb_eig_vectors_dev back-transforms Z where it lies: no n x n matrix crosses the bus.

The matrix never visits the host when it is built there (make_grm(eigen_solver="device")), and K need not either (keep_on_device=True):
Context.poly_setup() borrows it where it lies."""
import ctypes as C

import numpy as np

from ._lib import HibayesError, check, lib


def tridiagonal_eigh(d, e):
    """Stage 2 on the host: LAPACK dstemr through scipy, eigenvalues ascending. n = 1 has nothing to solve."""
    d = np.asarray(d, dtype=np.float64)
    if d.size == 1:
        return d.copy(), np.ones((1, 1), order="F")
    from scipy.linalg import eigh_tridiagonal
    w, Z = eigh_tridiagonal(d, np.asarray(e, dtype=np.float64), lapack_driver="stemr")
    return w, np.asfortranarray(Z)


def check_tridiagonal(who, tridiagonal, eigen_solver="device"):
    if tridiagonal not in ("host", "device"):
        raise ValueError("%s: tridiagonal must be \"host\" or \"device\", not %r" % (who, tridiagonal))
    if tridiagonal == "device" and eigen_solver != "device":
        raise ValueError("%s: tridiagonal=\"device\" goes with eigen_solver=\"device\"" % who)


def tridiagonal_eigh_device(d, e, device=0):
    """Stage 2 on the device: (w ascending, Z as a DeviceMatrix whose column j belongs to w[j]) of tridiag(e, d, e), by hb_eig_tridiagonal."""
    d = np.ascontiguousarray(d, dtype=np.float64).ravel()
    n = d.size
    e = np.zeros(0) if e is None else np.ascontiguousarray(e, dtype=np.float64).ravel()
    if n < 1 or e.size != max(n - 1, 0):
        raise ValueError("tridiagonal_eigh_device: d must hold n >= 1 values and e n - 1")
    w = np.zeros(n)
    Z, ldz = C.c_void_p(), C.c_int64()
    check(lib().hb_eig_tridiagonal(d.ctypes.data, e.ctypes.data if n > 1 else None, n, int(device), w.ctypes.data, C.byref(Z), C.byref(ldz)))
    return w, DeviceMatrix(Z.value, n, ldz.value, device)


def stedc_plan(n, splits=()):
    """The merge tree hb_eig_tridiagonal uses (hb_stedc_plan; needs no device): dict(leaf_rows, levels, leaves [(lo, hi)], merges [(lo, mid, hi,
    level)])."""
    sp = np.ascontiguousarray(splits, dtype=np.int32)
    cap = max(int(n), 1)
    a = [np.zeros(cap, dtype=np.int32) for _ in range(6)]
    cnt = [C.c_int32() for _ in range(4)]
    check(lib().hb_stedc_plan(int(n), sp.ctypes.data if sp.size else None, int(sp.size), cap, a[0].ctypes.data, a[1].ctypes.data,
                              C.addressof(cnt[0]), a[2].ctypes.data, a[3].ctypes.data, a[4].ctypes.data, a[5].ctypes.data, C.addressof(cnt[1]),
                              C.addressof(cnt[2]), C.addressof(cnt[3])))
    nl, nm = cnt[0].value, cnt[1].value
    return dict(leaf_rows=cnt[3].value, levels=cnt[2].value, leaves=[(int(a[0][i]), int(a[1][i])) for i in range(nl)],
                merges=[(int(a[2][i]), int(a[3][i]), int(a[4][i]), int(a[5][i])) for i in range(nm)])


def stedc_stats():
    """The phases of this process's last tridiagonal_eigh_device, in seconds, and its GEMM's floating-point operations (tools/eig_timing.py)"""
    v = np.zeros(6)
    check(lib().hb_stedc_stats(v.ctypes.data, 6))
    return dict(leaves=v[0], scan=v[1], secular=v[2], gemm=v[3], copies=v[4], gemm_flops=v[5])


class DeviceMatrix:
    """An n x n fp64 matrix on the device (column-major, leading dimension `ld`) that this object owns: .toarray() downloads it, .close()
    frees it."""

    def __init__(self, ptr, n, ld, device, free="hb_eig_release"):
        self.ptr, self.n, self.ld, self.device, self._free = ptr, int(n), int(ld), int(device), free

    @property
    def shape(self):
        return (self.n, self.n)

    def _live(self, who):
        if not self.ptr:
            raise HibayesError(1, "%s: the device matrix has been closed" % who)

    def toarray(self):
        self._live("toarray")
        out = np.zeros((self.n, self.n), order="F")
        check(lib().hb_eig_download(self.ptr, self.ld, self.n, self.device, out.ctypes.data, self.n))
        return out

    def close(self):
        if self.ptr:
            getattr(lib(), self._free)(self.ptr)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EigVectors(DeviceMatrix):
    """The eigenvectors K on the device with their eigenvalues `.values` (ascending, column j of K belongs to values[j]). `.ld` is even, so every
    column is 16-byte aligned: Context.poly_setup(values, handle) borrows the matrix and keeps this object alive."""

    def __init__(self, values, ptr, n, ld, device):
        super().__init__(ptr, n, ld, device)
        self.values = values


class Reduction:
    """hb_eig_reduce on a device matrix: .d, .e (the tridiagonal matrix, host), then .vectors(Z) -> EigVectors, .reflectors() -> (A as dsytrd
    leaves it, tau). Borrows `A` (a DeviceMatrix, kept alive) until .close()."""

    def __init__(self, A):
        A._live("Reduction")
        self.A, self.n, self.device = A, A.n, A.device
        self.d, self.e = np.zeros(self.n), np.zeros(max(self.n - 1, 0))
        h = C.c_void_p()
        check(lib().hb_eig_reduce(A.ptr, A.ld, A.n, A.device, self.d.ctypes.data, self.e.ctypes.data if self.n > 1 else None, C.byref(h)))
        self.h = h

    def _live(self, who):
        if not self.h:
            raise HibayesError(1, "%s: the reduction has been closed" % who)

    def vectors(self, Z=None, values=None):
        """K = Q Z on the device (Z = None: Q itself)"""
        self._live("vectors")
        Zf = None if Z is None else np.asfortranarray(Z, dtype=np.float64)
        if Zf is not None and Zf.shape != (self.n, self.n):
            raise ValueError("vectors: Z must be n x n")
        K, ldk = C.c_void_p(), C.c_int64()
        check(lib().hb_eig_vectors(self.h, None if Zf is None else Zf.ctypes.data, self.n, C.byref(K), C.byref(ldk)))
        return EigVectors(values, K.value, self.n, ldk.value, self.device)

    def vectors_dev(self, Zdev, values=None):
        """K = Q Z in place in the DeviceMatrix Zdev (tridiagonal_eigh_device's), which is taken over: it is closed, the EigVectors owns the buffer"""
        self._live("vectors_dev")
        Zdev._live("vectors_dev")
        if Zdev.n != self.n or Zdev.device != self.device:
            raise ValueError("vectors_dev: Z must be n x n on the reduction's device")
        K, ldk = C.c_void_p(), C.c_int64()
        check(lib().hb_eig_vectors_dev(self.h, Zdev.ptr, Zdev.ld, C.byref(K), C.byref(ldk)))
        Zdev.ptr = None
        return EigVectors(values, K.value, self.n, ldk.value, self.device)

    def reflectors(self):
        self._live("reflectors")
        tau = np.zeros(max(self.n - 1, 0))
        if self.n > 1:
            check(lib().hb_eig_tau(self.h, tau.ctypes.data))
        return self.A.toarray(), tau

    def close(self):
        if self.h:
            lib().hb_eig_destroy(self.h)
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


def upload(A, device=0, lda=None):
    """A symmetric host matrix on the device (only its lower triangle will be read). `lda` (tests): refuse like the library does."""
    A = np.asfortranarray(A, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("eigh: A must be a square matrix")
    n = A.shape[0]
    p, ld = C.c_void_p(), C.c_int64()
    check(lib().hb_eig_upload(A.ctypes.data, n if lda is None else int(lda), n, int(device), C.byref(p), C.byref(ld)))
    return DeviceMatrix(p.value, n, ld.value, device)


def eigh_device(A, keep_on_device=False, stats=None, tridiagonal="host"):
    """(values, vectors) of the DeviceMatrix A, which is overwritten and closed. `stats` (a dict) receives the stages' seconds. tridiagonal:
    "host" (dstemr) or "device" (tridiagonal_eigh_device; Z is back-transformed where it lies)."""
    import time
    check_tridiagonal("eigh", tridiagonal)
    t0 = time.perf_counter()
    try:
        with Reduction(A) as red:
            t1 = time.perf_counter()
            if tridiagonal == "device":
                w, Zdev = tridiagonal_eigh_device(red.d, red.e, red.device)
                t2 = time.perf_counter()
                with Zdev:
                    K = red.vectors_dev(Zdev, w)
            else:
                w, Z = tridiagonal_eigh(red.d, red.e)
                t2 = time.perf_counter()
                K = red.vectors(Z, w)
            t3 = time.perf_counter()
    finally:
        A.close()
    if stats is not None:
        stats.update(reduce=t1 - t0, tridiagonal=t2 - t1, vectors=t3 - t2)
    if keep_on_device:
        return K
    with K:
        return w, K.toarray()


def eigh(A, *, device=0, keep_on_device=False, tridiagonal="host"):
    """Eigenvalues (ascending) and eigenvectors of the symmetric host matrix A, as numpy.linalg.eigh(A) returns them (UPLO = "L"), with the
    reduction to tridiagonal form and the back-transformation on the device. keep_on_device=True returns an EigVectors handle (.values, .shape,
    .ld, .toarray(), .close()) instead of the pair: the vectors stay on the device. tridiagonal="device" solves the tridiagonal stage on the
    device as well (divide and conquer) instead of with LAPACK dstemr on the host."""
    check_tridiagonal("eigh", tridiagonal)
    return eigh_device(upload(A, device), keep_on_device, tridiagonal=tridiagonal)
