"""Host mirror of the reference's ldmat() (R/ldm.r:31-112): argument handling on the host, the matrix itself on the device
through hb_ldm_build (include/hibayes_gpu.h; tXXmat_Geno / tXXmat_Chr, src/tXXmat.cpp:100-206, :504-626). There is no CPU
fallback."""
import ctypes as C

import numpy as np

from ._lib import LdmStats, check, lib
from .engine import Context

KINDS = ("dense", "sparse", "block-dense", "block-sparse")


class LDMatrix:
    """A finished LD matrix kept with the library (hb_ldm): SBayesD() and sbrm() take it as `ldm` and run from its dense device
    copy, SBayesS() and sbrm(sparse_ld=True) from its device CSC, so .bed -> ldmat -> sbrm needs no host matrix. toarray() /
    tocsc() download it."""

    def __init__(self, handle, device=0):
        self.L, self.h, self.device = lib(), handle, device
        st = self.info()
        self.shape = (st["m"], st["m"])
        self.kind, self.nnz = KINDS[st["kind"]], st["nnz"]

    @classmethod
    def from_scipy(cls, mat, device=0):
        """A handle (kind "sparse") from a scipy sparse matrix, for SBayesS(): converted to CSC with sorted, summed indices and
        handed to hb_ldm_from_csc, which refuses a matrix that does not equal its transpose in pattern and in value bits."""
        import scipy.sparse as sp
        if not sp.issparse(mat) or mat.ndim != 2 or mat.shape[0] != mat.shape[1]:
            raise ValueError("from_scipy needs a square scipy sparse matrix")
        A = sp.csc_matrix(mat, dtype=np.float64, copy=True)
        A.sum_duplicates()
        A.sort_indices()
        indptr, indices = np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int32)
        data = np.ascontiguousarray(A.data, dtype=np.float64)
        h = C.c_void_p()
        check(lib().hb_ldm_from_csc(A.shape[0], indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, int(device), C.byref(h)))
        return cls(h, device)

    def info(self):
        s = LdmStats()
        check(self.L.hb_ldm_info(self._handle(), C.byref(s)))
        return {k: getattr(s, k) for k, _ in LdmStats._fields_}

    def _handle(self):
        if not self.h:
            raise ValueError("this LDMatrix was closed")
        return self.h

    def toarray(self):
        m = self.shape[0]
        out = np.zeros((m, m), order="F")
        check(self.L.hb_ldm_download_dense(self._handle(), out.ctypes.data, m))
        return out

    def tocsc(self):
        import scipy.sparse as sp
        if self.kind == "dense":
            return sp.csc_matrix(self.toarray())
        m = self.shape[0]
        indptr, indices, data = np.zeros(m + 1, dtype=np.int64), np.zeros(self.nnz, dtype=np.int32), np.zeros(self.nnz)
        check(self.L.hb_ldm_download_csc(self._handle(), indptr.ctypes.data, indices.ctypes.data, data.ctypes.data))
        return sp.csc_matrix((data, indices, indptr), shape=self.shape)

    def window_var(self, A, windindx, nw=None):
        """(var, total): var[w - 1, r] = alpha_w,r' V_ww alpha_w,r over the stored entries of the matrix for every window id w of windindx (m ids
        in 1 .. nw) and every record r (column of A, m x R), total[r] = alpha_r' V alpha_r. On the device from the copy the handle's kind reads
        (hb_ldm_window_var); hibayes_amd.ld_window_pve() makes PVE and WPPA of them. Nothing is clamped: a thresholded matrix is indefinite and
        a form may be negative. nw: the number of windows where it is more than the largest id used (the rows past it, like every window
        without an effect, are 0.0)."""
        m = self.shape[0]
        A = np.asfortranarray(A, dtype=np.float64)
        if A.ndim == 1:
            A = A.reshape(-1, 1, order="F")
        if A.ndim != 2:
            raise ValueError("A must be (m,) or (m, R)")
        wi = np.asarray(windindx)
        if wi.shape != (m,) or wi.dtype.kind not in "iu":
            raise ValueError("windindx must hold one integer window id per marker")
        if wi.min() < 1:
            raise ValueError("windindx must hold window ids in 1 .. nw")
        nw = int(wi.max()) if nw is None else int(nw)
        if nw < wi.max():
            raise ValueError("windindx must hold window ids in 1 .. nw")
        wi = np.ascontiguousarray(wi, dtype=np.uint32)
        var, total = np.zeros((nw, A.shape[1]), order="F"), np.zeros(A.shape[1])
        check(self.L.hb_ldm_window_var(self._handle(), A.ctypes.data, max(A.shape[0], 1), A.shape[0], A.shape[1], wi.ctypes.data, nw, var.ctypes.data, nw,
                                       total.ctypes.data))
        return var, total

    def diagonal(self):
        """The m diagonal entries, from the copy the handle's kind reads (hb_ldm_diagonal); 0.0 where a sparse matrix stores none."""
        out = np.zeros(self.shape[0])
        check(self.L.hb_ldm_diagonal(self._handle(), out.ctypes.data))
        return out

    def close(self):
        if self.h:
            self.L.hb_ldm_destroy(self.h)
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


def _isna(v):
    return v is None or (isinstance(v, float) and np.isnan(v)) or (isinstance(v, str) and v in ("NA", ""))


def _tonum(v):
    try:
        return float(v)
    except (TypeError, ValueError):
        return None


def _map_snp_chr(map):
    """Columns 1 and 2 (SNP, chromosome) of `map`: a table, or the dict read_plink() returns."""
    if isinstance(map, dict):
        sk = next((k for k in ("SNP", "snp") if k in map), None)
        ck = next((k for k in ("Chr", "chr", "CHROM", "chrom") if k in map), None)
        if sk is None or ck is None:
            raise ValueError("map needs the columns SNP and chromosome")
        return list(map[sk]), list(map[ck])
    arr = np.asarray(map, dtype=object)
    if arr.ndim != 2 or arr.shape[1] < 2:
        raise ValueError("map needs the columns SNP and chromosome")
    return list(arr[:, 0]), list(arr[:, 1])


def chromosome_ids(chr_raw):
    """R/ldm.r:66-75: numeric labels keep their value, every other label becomes max.chr + 1, + 2, ... in order of appearance."""
    num = [_tonum(v) for v in chr_raw]
    known = [v for v in num if v is not None and not np.isnan(v)]
    max_chr = max(known) if known else 0
    inrange = lambda v: v is not None and v == int(v) and 0 <= v <= max_chr
    extra, out = {}, []
    for raw, v in zip(chr_raw, num):
        if inrange(v):
            out.append(int(v))
        else:
            if raw not in extra:
                extra[raw] = int(max_chr) + len(extra) + 1
            out.append(extra[raw])
    return np.array(out, dtype=np.int32)


def ldmat_mode(m, map=None, gwas_geno=None, gwas_map=None, chisq=None, ldchr=False):
    """The host part of ldmat(), R/ldm.r:44-92: returns (chr ids or None for the genome-wide matrix, chisq or None)."""
    if chisq is not None and chisq < 0:                               # :44-46
        chisq = None
    chr_ids = None
    if map is not None:
        snp, chr_raw = _map_snp_chr(map)
        single = len(set(chr_raw)) == 1
        if single:                                                    # :51
            ldchr = True
        if chisq is not None and chisq == 0 and single:               # :52-54
            chisq = None
        if len(set(snp)) != len(snp):                                 # :55
            raise ValueError("Same SNPs names detected.")
        if any(_isna(v) for v in chr_raw):                            # :56-60
            raise ValueError("NAs are not allowed in chromosome.")
        if any(_tonum(v) == 0 for v in chr_raw):                      # :61-63
            raise ValueError("0 is not allowed in chromosome.")
        if len(snp) != m:
            raise ValueError("map must have one row per marker of geno")
        chr_ids = chromosome_ids(chr_raw)
    else:
        if chisq is not None and chisq == 0:                          # :78-80
            chisq = None
        ldchr = True                                                  # :81
    if gwas_map is not None:                                          # :83-85
        gs = _map_snp_chr(gwas_map)[0]
        if len(set(gs)) != len(gs):
            raise ValueError("Same SNPs names detected.")
    if gwas_geno is not None:
        raise NotImplementedError("gwas_geno (tXXmat_Geno_gwas / tXXmat_Chr_gwas and their sparse forms) is outside the GPU path")
    return (None if ldchr else chr_ids), (None if chisq is None else float(chisq))   # :87-92


def ldmat(geno, map=None, gwas_geno=None, gwas_map=None, chisq=None, ldchr=False, threads=4, verbose=False, *, device=0,
          keep_on_device=False, strip_bytes=0):
    """ldmat() of the reference (R/ldm.r:31-112) on the device. geno: an int8 array (n x m), a float array of integer codes
    (checked like Context.upload), or a Context that already holds genotypes (e.g. after upload_bed). map: table with the
    columns SNP, chromosome, position, or read_plink()'s dict. As in the reference `ldchr=True` (or no map, or one chromosome)
    gives the genome-wide matrix, `ldchr=False` with a map one block per chromosome.

    Returns the genome-wide dense matrix as a Fortran-order numpy array and every other result — chisq-sparsified or per
    chromosome — as scipy.sparse.csc_matrix (the reference returns sp_mat there); with keep_on_device=True an LDMatrix that
    SBayesD() / sbrm() accept as `ldm`. Every entry equals the reference's bit for bit. The four variants with a second
    genotype sample (gwas_geno; tXXmat_*_gwas) are out of scope and raise NotImplementedError. threads is accepted and ignored."""
    own = None
    if isinstance(geno, Context):
        ctx = geno
        m = ctx.m
    else:
        X = np.asarray(geno)
        if X.ndim != 2:
            raise ValueError("geno must be an n x m matrix")
        m = X.shape[1]
    chr_ids, chisq = ldmat_mode(m, map, gwas_geno, gwas_map, chisq, ldchr)
    if verbose:
        print(("Genome-Wide" if chr_ids is None else "Chromosome-Wide") +
              (" sparse matrix" if (chisq is not None and (chr_ids is not None or chisq > 0)) else " dense matrix"))
    try:
        if not isinstance(geno, Context):
            ctx = own = Context(X.shape[0], m, device=device)
            ctx.upload(X)
        ld = ctx.ldmat(chr_ids, chisq, strip_bytes=strip_bytes)
    finally:
        if own is not None:
            own.close()
    if keep_on_device:
        return ld
    with ld:
        return ld.toarray() if ld.kind == "dense" else ld.tocsc()
