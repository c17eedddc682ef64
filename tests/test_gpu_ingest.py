"""The data paths either side of the genotype matrix (hibayes_amd/csrc/hb_ingest.hpp, drivers in hb_ctx.hip) at their edges: X alpha
(k_xalpha) and the GEBV sample matrix (k_xmat) on the int8 and the 2-bit layout, bit for bit against tests/ingest_restatement.py where
the kernel's order is fixed and within the derived bound of the exactly rounded product where it is free; the float upload (k_f64_to_i8) at
its range's ends, from a strided source, into a column range and over two staging chunks; the .bed decode (k_bed_decode) on crafted
markers; the generator's (k_generate) second trip over the columns. Every tolerance is an equality or k eps sum |terms|."""
import functools
import time

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd import plink
from hibayes_amd.engine import Context
from oracle import oracle as O
import ingest_restatement as I

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
NS = [2, 255, 257, 1025]          # ld = 256, 256, 512, 1280; the last live thread (four rows each) owns one, three, one and one rows
REFUSED = "genotype matrix holds non-integer or out-of-range values"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- data ----
def codes(rng, n, m, kind):
    """kind 2: codes 0..2; 3: codes 0..3 (the 2-bit layout's fourth code at each of a word's 16 positions where n allows it, and a column that is
    all 3); -1: int8 only, -127, -1, 0, 1, 2 and 127. Row 0 is all zero: its products vanish whatever the effects."""
    p = rng.uniform(0.05, 0.5, m)
    X = sum((rng.random((n, m)) < p).astype(np.int8) for _ in range(3 if kind == 3 else 2))
    if kind == 3:
        X[:16, 2] = 3
        X[:, 1] = 3
    if kind == -1:
        X = np.where(rng.random((n, m)) < 0.3, rng.choice(np.array([-127, -1, 127], dtype=np.int8), size=(n, m)), X)
    X[0, :] = 0
    X[n - 1, :] = np.where(X[n - 1, :] == 0, 1, X[n - 1, :])      # the last live row meets every effect
    X = np.asfortranarray(X.astype(np.int8))
    if kind == 3:
        assert X.min() == 0 and X.max() == 3
    if kind == -1:
        assert all((X == v).any() for v in (-127, -1, 127))
    return X


def effect_vectors(rng, m):
    """(name, alpha) for X alpha: 0, 1, 5 and 40 non-zeros over the first two column blocks, every non-zero in the second block, a -0.0 with
    denormals alone, and the same among ordinary effects"""
    out = []
    for nnz in (0, 1, 5, 40):
        a = np.zeros(m)
        cols = np.concatenate([rng.choice(256, nnz // 2, replace=False), 256 + rng.choice(m - 256, nnz - nnz // 2, replace=False)])
        a[cols.astype(np.int64)] = rng.normal(size=nnz) * 10.0 ** rng.integers(-3, 4, nnz)
        out.append(("nnz=%d" % nnz, a))
    if m > 512:                                        # three blocks and more: some effects past the second one too
        out[3][1][512 + rng.choice(m - 512, 9, replace=False)] = rng.normal(size=9)
    a = np.zeros(m)
    a[256 + rng.choice(min(m, 512) - 256, 7, replace=False)] = rng.normal(size=7)
    out.append(("second block only", a))
    a = np.zeros(m)
    a[3], a[10], a[290] = -0.0, 1e-310, -3e-320
    out.append(("-0.0 and denormals alone", a))
    a = a.copy()
    a[20], a[270] = 0.37, -1e-300
    out.append(("-0.0 and denormals among others", a))
    return out


def matvec(c, alpha):
    """hb_ctx_matvec into a vector that holds NaN before the call: a row the call never wrote stays one"""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    out = np.full(c.n, np.nan)
    H._lib.check(c.L.hb_ctx_matvec(c.h, alpha.ctypes.data, out.ctypes.data))
    return out


# ---- 1. X alpha ----
@pytest.mark.parametrize("m", [300, 700])
@pytest.mark.parametrize("n", NS)
def test_xalpha_on_the_int8_and_the_two_bit_layout(n, m):
    """hb_ctx_matvec (k_xalpha) at panel 64. m = 300: m_pad 320, two column blocks, the second ragged. Each block's sum is one chain of fused
    multiply-adds in ascending column order (xalpha_blocks), the sums meet in atomics on a zeroed vector and a zero sum is not sent: a row is
    fl(p0 + p1) in either order — equal bits, on both layouts and between two calls. m = 700: m_pad 704, three blocks, the atomics' order is
    free: |out - exact| <= nnz eps sum |x| |alpha| (a term goes through at most nnz roundings: its block's chain, then the blocks' additions).
    A row of zero genotypes is +0.0, the whole vector is +0.0 without effects, and no row of the NaN-filled output is left unwritten."""
    rng = np.random.default_rng(1000 * n + m)
    m_pad = -(-m // 64) * 64
    for kind in (2, 3, -1):
        X = codes(rng, n, m, kind)
        absX = np.abs(X.astype(np.float64))
        with Context(n, m, panel=64) as c:
            c.upload(X)
            layouts = [8] if kind == -1 else [8, 2]
            first = {}
            for layout in layouts:
                if layout == 2:
                    c.set_layout(2, keep_int8=False)
                    assert c.layout() == (2, False)
                rng_a = np.random.default_rng(n + m + kind)       # the same effects on both layouts
                for name, alpha in effect_vectors(rng_a, m):
                    tag = (n, m, kind, layout, name)
                    out = matvec(c, alpha)
                    out2 = matvec(c, alpha)
                    assert not np.isnan(out).any(), tag
                    nnz = int((alpha != 0.0).sum())
                    want = I.exact_dot(X, alpha)
                    lim = nnz * EPS * (absX @ np.abs(alpha))
                    err = np.abs(out - want)
                    print("%s: max err / bound = %.3g" % (tag, np.max(err / np.maximum(lim, 5e-324))))
                    assert np.all(err <= lim), tag
                    assert out[0] == 0.0 and not np.signbit(out[0]), tag
                    if nnz == 0:
                        assert not out.any() and not np.signbit(out).any(), tag
                    else:
                        assert out[n - 1] != 0.0, tag
                    if m == 300:
                        p = I.xalpha_blocks(X, alpha, m_pad)
                        assert p.shape[0] == 2
                        assert np.array_equal(bits(out), bits(p[0] + p[1])), tag
                        assert np.array_equal(bits(out), bits(out2)), tag
                        if layout == 2:
                            assert np.array_equal(bits(out), bits(first[name])), tag
                        first[name] = out


# ---- 2. the GEBV sample matrix ----
@pytest.mark.parametrize("n", NS)
def test_xmat_on_the_int8_and_the_two_bit_layout(n):
    """Context.matmul (hb_ctx_matmul, k_xmat) at m = 300, panel 64. No atomics: per record acc = 0; acc = fma(x_j, A[j, r], acc) over the
    columns that carry a non-zero in any of the pass's eight records, ascending (xmat_pass) — equal bits for every record, on both layouts and
    between two calls. 1, 8, 9 and 17 records with supports of 5 | 6 | 7, 8 | 41, 0, 3 columns: nnz % 4 = 1, 2, 3, 0 (the last batch of four
    reads its columns through idx[min(e0 + k, nnz - 1)]), a pass of eight empty records (k_xmat with nnz = 0) inside R = 17 and alone. A record
    computed alone has its own, smaller support; inside its pass the zeros of the larger support are walked too, which xmat_pass says changes
    no bit (acc + 0 x = acc, and acc is never -0.0): both are held to xmat_pass, and to each other. Against the exactly rounded product
    within max(1, |support|) eps sum |x| |a|."""
    rng = np.random.default_rng(n)
    m = 300
    for kind in (2, 3, -1):
        X = codes(rng, n, m, kind)
        absX = np.abs(X.astype(np.float64))
        cases = []
        for R, sizes in ((1, [5]), (8, [6]), (9, [7, 8]), (17, [41, 0, 3])):
            A = np.zeros((m, R))
            for b, k in enumerate(sizes):
                cols = rng.choice(m, k, replace=False)
                recs = np.arange(8 * b, min(R, 8 * b + 8))
                for j in cols:                              # every column of the pass's set in one of its records at least, in half of the others
                    on = rng.random(recs.size) < 0.5
                    on[rng.integers(recs.size)] = True
                    A[j, recs[on]] = rng.normal(size=int(on.sum())) * 10.0 ** rng.integers(-3, 4)
                if recs.size > 1 and k:                     # the pass's first record misses one of the pass's columns
                    A[cols[0], recs[0]], A[cols[0], recs[1]] = 0.0, rng.normal()
                assert ((A[:, recs] != 0).any(axis=1)).sum() == k
            if R == 9:                                      # a -0.0 is no non-zero by the support rule: its column stays out of pass 0
                A[np.flatnonzero(~(A[:, :8] != 0).any(axis=1))[0], 3] = -0.0
            cases.append((R, sizes, A))
        cases.append((8, [0], np.zeros((m, 8))))
        with Context(n, m, panel=64) as c:
            c.upload(X)
            for layout in ([8] if kind == -1 else [8, 2]):
                if layout == 2:
                    c.set_layout(2, keep_int8=False)
                    assert c.layout() == (2, False)
                smaller = 0
                for R, sizes, A in cases:
                    tag = (n, kind, layout, R)
                    out = c.matmul(A)
                    assert np.array_equal(bits(out), bits(c.matmul(A))), tag
                    for b in range(len(sizes)):
                        support, want = I.xmat_pass(X, A, 8 * b)
                        assert support.size == sizes[b]
                        assert np.array_equal(bits(out[:, 8 * b:8 * b + 8]), bits(want)), tag + (b,)
                        for k in range(want.shape[1]):
                            r = 8 * b + k
                            lim = max(1, support.size) * EPS * (absX @ np.abs(A[:, r]))
                            assert np.all(np.abs(out[:, r] - I.exact_dot(X, A[:, r])) <= lim), tag + (r,)
                        if R >= 8 and support.size:         # the pass's first record alone
                            r = 8 * b
                            alone = c.matmul(A[:, r])
                            s1, w1 = I.xmat_pass(X, A[:, r:r + 1], 0)
                            smaller += s1.size < support.size
                            assert np.array_equal(bits(alone[:, 0]), bits(w1[:, 0])), tag + (r, "alone")
                            assert np.array_equal(bits(alone[:, 0]), bits(out[:, r])), tag + (r, "alone and in its pass")
                    if R == 17:
                        assert not out[:, 8:16].any() and not np.signbit(out[:, 8:16]).any()
                    if sizes == [0]:
                        assert not out.any() and not np.signbit(out).any()
                    assert not out[0].any()                 # the row of zero genotypes
                assert smaller >= 3


# ---- 3. the float upload ----
def float_matrix(seed=3, n=257, m=70):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.integers(0, 3, size=(n, m)).astype(np.float64))


def test_float_upload_at_the_ends_of_its_range():
    """k_f64_to_i8 takes the integers of [-127, 127], a -0.0 as 0; everything else — a half, -128 and 128, what is not finite, what no int8 could
    hold, the double below 1 — is refused with status 4, also as the only such value of the matrix at its last row and column."""
    n, m = 257, 70
    X = float_matrix()
    X[0, 0], X[1, 0], X[2, 0], X[3, 0] = -127.0, 127.0, -0.0, 2.0
    X[n - 1, m - 1], X[n - 2, m - 1], X[n - 1, 0] = -127.0, 127.0, -0.0
    with Context(n, m, panel=64) as c:
        c.upload(X)
        back = c.download()
        assert back.dtype == np.int8 and np.array_equal(back, X.astype(np.int8))
        assert back[0, 0] == -127 and back[1, 0] == 127 and back[2, 0] == 0 and back[n - 1, m - 1] == -127 and back[n - 1, 0] == 0
        for v in (127.5, -128.0, 128.0, np.nan, np.inf, -np.inf, 1e300, 0.9999999999999999):
            bad = X.copy()
            bad[n - 1, m - 1] = v
            with pytest.raises(H.HibayesError) as ei:
                c.upload(bad)
            assert ei.value.status == 4 and REFUSED in str(ei.value), v
        c.upload(X)                                         # the context takes a good matrix after the refusals
        assert np.array_equal(c.download(), X.astype(np.int8))


def test_float_upload_from_a_strided_source():
    """hb_ctx_upload_genotype_f64 with ld above n: rows 7 .. 7 + n of a taller Fortran array whose other rows hold 0.5, which the upload refuses
    wherever it reads one. The same bytes as the contiguous copy."""
    n, m = 257, 70
    X = float_matrix(4)
    T = np.full((n + 43, m), 0.5, order="F")
    T[7:7 + n] = X
    S = T[7:7 + n]
    assert S.strides == (8, 8 * (n + 43)) and not S.flags.f_contiguous
    with Context(n, m, panel=64) as c:
        c.upload(X)
        want = c.download()
        c.upload(np.zeros((n, m), dtype=np.int8))
        assert not c.download().any()
        H._lib.check(c.L.hb_ctx_upload_genotype_f64(c.h, S.ctypes.data, n + 43, 0, m))
        got = c.download()
    assert np.array_equal(got, X.astype(np.int8)) and got.tobytes() == want.tobytes()


def test_float_upload_into_a_column_range():
    """A float block with col0 > 0: X is the address of the block's first column for both upload calls (include/hibayes_gpu.h). The float
    driver used to add col0 columns to it once more and read past the caller's block. Ten new columns over 60 .. 69 of a resident int8
    matrix: they arrive, 0 .. 59 stay, and the padding rows n .. ld of the touched columns are still zero — xpx, summed over ld rows, is the exact
    integer."""
    n, m = 257, 70
    rng = np.random.default_rng(5)
    X8 = np.asfortranarray(rng.integers(0, 3, size=(n, m)).astype(np.int8))
    F = np.asfortranarray(rng.choice([-127.0, -1.0, 0.0, 1.0, 2.0, 3.0, 127.0], size=(n, m)))
    block = F[:, 60:70]
    assert block.flags.f_contiguous and block.ctypes.data == F.ctypes.data + 8 * 60 * n
    assert (block != X8[:, 60:70]).mean() > 0.5
    want = X8.copy()
    want[:, 60:70] = block.astype(np.int8)
    with Context(n, m, panel=64) as c:
        c.upload(X8)
        c.upload(block, col0=60)
        got = c.download()
        xpx = c.marker_stats()[0]
        assert np.array_equal(c.download(60, 10), want[:, 60:70])
    assert np.array_equal(got[:, 60:], want[:, 60:])
    assert np.array_equal(got[:, :60], X8[:, :60])
    assert np.array_equal(xpx, (want.astype(np.int64) ** 2).sum(0).astype(np.float64))


def test_float_upload_over_two_staging_chunks():
    """hb_ctx_upload_genotype_f64 stages chunk = max(1, min(ncols, 2^26 / n)) columns at a time. n = 1 048 577, m = 64 is the smallest case with two
    chunks and a ragged last one: 63 columns, then 1. Allocates a 537 MB host matrix, 67 MB of int8 on the device (ld = 1 048 832) and a
    528 MB staging buffer there for the length of each upload. Column j holds (i + j) % 3; columns 0, 62 and 63 come back as they went. Then a 0.5
    in column 63, the second chunk: refused. Two uploads; the time of the whole test is printed (measured on the MI355X: 0.23 s)."""
    t0 = time.perf_counter()
    n, m = (1 << 20) + 1, 64
    assert min(m, (1 << 26) // n) == 63
    X = np.empty((n, m), order="F")
    i = np.arange(n, dtype=np.int64)
    for j in range(m):
        X[:, j] = (i + j) % 3
    with Context(n, m, panel=64) as c:
        c.upload(X)
        for j in (0, 62, 63):
            assert np.array_equal(c.download(j, 1)[:, 0], ((i + j) % 3).astype(np.int8)), j
        X[n - 1, 63] = 0.5
        with pytest.raises(H.HibayesError) as ei:
            c.upload(X)
        assert ei.value.status == 4 and REFUSED in str(ei.value)
    print("two uploads of %d x %d doubles: %.1f s in all" % (n, m, time.perf_counter() - t0))


# ---- 4. .bed decode ----
def row_lists(nind, rng):
    """(name, rows, selected): None = the first n of nind, n = nind - 2, so that the counts run over individuals that are not written"""
    n = nind - 2
    perm = rng.permutation(nind)[:n]
    rep = perm.copy()
    rep[-1] = rep[0]
    return [("first n", None, np.arange(n)), ("permutation", perm, perm), ("reversed", np.arange(nind - 1, -1, -1)[:n], np.arange(nind - 1, -1, -1)[:n]),
            ("repeated index", rep, rep)]


@pytest.mark.parametrize("nind", [5, 6, 7, 8, 255, 1003])
def test_bed_decode_on_crafted_markers(nind):
    """hb_ctx_upload_bed (k_bed_decode) on the twelve markers of ingest_restatement.bed_markers — ties between the counts, a marker that is
    missing everywhere, missing calls only among the individuals that are not selected — with n = nind - 2 rows: the first n, a permutation, a
    reversed list and one with a repeated index; nind % 4 = 1, 2, 3, 0, fewer individuals than the workgroup's 256 threads and more. Each image
    twice, the unused bit pairs of every marker's last byte all 00 (genotype 2 to a count that ran past nind) and all 01: the same columns.
    Reference: plink.decode_bed(...)[rows], which tests/test_ingest_host.py holds to the oracle's decoder and to the reference's rule. Then the
    columns 3 .. 7 alone, from an image that ends with marker 7, into a context that holds other genotypes; and the refusals."""
    rng = np.random.default_rng(nind)
    n = nind - 2
    bpc = (nind + 3) // 4
    for name, rows, sel in row_lists(nind, rng):
        outside = np.setdiff1d(np.arange(nind), sel)
        assert outside.size >= 2
        G = I.bed_markers(nind, inside=int(sel[n // 2]), outside=outside, seed=nind)
        assert not (G[sel, 6] == I.NA).any() and (G[outside, 6] == I.NA).all()
        images = [I.bed_image(G, nind, tail) for tail in (0, 1)]
        ref = plink.decode_bed(images[0], nind, I.BED_NSNP)
        assert np.array_equal(ref, plink.decode_bed(images[1], nind, I.BED_NSNP))
        for j, major in enumerate(I.BED_MAJOR):
            if major is not None:
                assert ref[sel[n // 2], j] == major
        other = np.asfortranarray(rng.integers(3, 9, size=(n, I.BED_NSNP)).astype(np.int8))
        with Context(n, I.BED_NSNP, panel=64) as c:
            for tail, img in zip((0, 1), images):
                c.upload(other)
                c.upload_bed(img, nind, rows=rows)
                got = c.download()
                bad = np.argwhere(got != ref[sel])
                assert bad.size == 0, (nind, name, tail, bad[:5].tolist())
            # a column range
            c.upload(other)
            short = images[0][:3 + bpc * 8]
            c.upload_bed(short, nind, rows=rows, col0=3, ncols=5)
            got = c.download()
            assert np.array_equal(got[:, 3:8], ref[sel][:, 3:8]), (nind, name)
            assert np.array_equal(got[:, :3], other[:, :3]) and np.array_equal(got[:, 8:], other[:, 8:]), (nind, name)
            if rows is None:
                continue
            # refusals: nothing is written
            wrong = [(short[:-1], rows, "file image too short"), (b"\x6c\x1b\x00" + short[3:], rows, "magic 6c 1b 01")]
            for v in (nind, -1):
                r = np.array(rows).copy()
                r[n - 1] = v
                wrong.append((short, r, "row index out of range"))
            for img, r, text in wrong:
                with pytest.raises(H.HibayesError) as ei:
                    c.upload_bed(img, nind, rows=r, col0=3, ncols=5)
                assert ei.value.status == 1 and text in str(ei.value), (nind, name, text)
            assert np.array_equal(c.download(), got)
    # ... and without a row list
    with Context(n, I.BED_NSNP, panel=64) as c:
        for img, text in ((short[:-1], "file image too short"), (b"\x6c\x1b\x00" + short[3:], "magic 6c 1b 01")):
            with pytest.raises(H.HibayesError) as ei:
                c.upload_bed(img, nind, col0=3, ncols=5)
            assert ei.value.status == 1 and text in str(ei.value)


# ---- 5. the generator ----
def test_generator_on_its_second_trip_over_the_columns():
    """k_generate's grid has min(m, 32768) rows of blocks and walks the columns j = blockIdx.y, + gridDim.y, ...: at m = 32768 + 5 the columns
    from 32768 on are written by the second trip. n = 5 at panel 64 (ld = 256: about 8.4 MB resident), m_offset = 1000, mono_every = 7.
    Columns 0, 1, 32767, 32768, 32769 and m - 1 element by element against the documented Philox stream."""
    n, m, seed, off, mono = 5, 32768 + 5, 20240901, 1000, 7
    check = [0, 1, 32767, 32768, 32769, m - 1]
    with Context(n, m, panel=64, m_offset=off) as c:
        c.generate(seed, mono_every=mono)
        got = {j: c.download(j, 1)[:, 0] for j in check}
    live = 0
    for j in check:
        gj = off + j
        sub = (3 << 56) | gj
        pj = 0.05 + 0.45 * O.lib().hbo_philox_uniform(seed, sub, 0xFFFFFFFFFF)
        thr = int(pj * 65536.0)
        want = []
        for i in range(n):
            w = int(O.philox_block(seed, sub, i // 4)[i % 4])
            x = int((w & 0xFFFF) < thr) + int((w >> 16) < thr)
            want.append(0 if gj % mono == mono - 1 else x)
        assert got[j].tolist() == want, j
        live += any(want)
    assert (off + 0) % mono == mono - 1 and (off + 32768) % mono != mono - 1 and live >= 2
