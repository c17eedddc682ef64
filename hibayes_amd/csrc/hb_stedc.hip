// hb_stedc.hip — stage 2 of eigh() on the device: the eigenvalues w and eigenvectors Z of the symmetric tridiagonal matrix
// T = tridiag(e, d, e) by Cuppen's divide and conquer with Gu-Eisenstat vectors, as LAPACK's dstedc / dlaed0-4 (the reference reaches them
// through Armadillo's eig_sym "dc", src/rm.cpp:46-52). Z is built on the device in the layout hb_eig_vectors gives K, so hb_eig_vectors_dev
// back-transforms it where it lies and no n x n matrix crosses the bus. tests/stedc_restatement.py restates every step in numpy.
//
//   1. T is scaled by its max-norm and split wherever |e_i| <= eps sqrt(|d_i|) sqrt(|d_i+1|) (eps = 2^-53, LAPACK's); a 1 x 1 part keeps its entry.
//   2. hb_stedcplan.hpp: the merge tree of every part; every tear takes rho = |e_k| off d_k and d_k+1.
//   3. k_stedc_leaf     a workgroup (one wave) per leaf, all leaves in one launch: cyclic Jacobi on the block in LDS, padded to 32 x 32, 16
//                       disjoint rotations per step in round-robin order; a rotation is skipped where |a_pq| <= eps max|T_leaf| / 32
//   4. per level, all its merges in the same launches:
//      k_stedc_gather   z: the last row of Q1, the first row of Q2 times sign(e_k)
//      (host)           dlaed2's O(k) scan on the downloaded z and the eigenvalues: sort by d, deflate |rho z_i| <= tol and poles closer than tol
//      k_stedc_rot      the close poles' Givens rotations of Z's columns, a workgroup per merge, in the scan's order
//      k_stedc_secular  a lane per root: (origin pole, tau), every difference (d_j - d_origin) - tau; rational steps on the two neighbouring
//                       poles inside a bracket that is always kept, bisection where a step leaves it; dlaed4's stop test; STEDC_MAXIT at most
//      k_stedc_lowner   zhat from the roots, the product taken ratio by ratio (no partial product over- or underflows)
//      k_stedc_norm     1 / ||(zhat_j / delta_ij)_j|| per root, and the new eigenvalue
//      k_stedc_ubuild   a strip of STEDC_STRIP columns of U, transposed (the GEMM reads it along the roots)
//      k_stedc_gemm     Znew[:, roots of the strip] = Zold[:, undeflated] U on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), two half-height
//                       products: a column that lives in one child only is zero in the other child's rows and is left out there
//      k_stedc_copy     deflated columns, and the finished nodes that wait for a later level, into the other buffer
//   5. k_stedc_permute  the columns in ascending order of the unscaled eigenvalues, once
// No floating-point atomic; every sum's order is a function of n, the split points, STEDC_LEAF and STEDC_STRIP alone. Peak device memory: Z, one
// workspace of the same size, n x STEDC_STRIP doubles of U and a few n-vectors.
#include "hb_internal.hpp"
#include "hb_mma.hpp"
#include "hb_stedcplan.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>

#ifndef STEDC_STRIP
#define STEDC_STRIP 256 // columns of U built and consumed at a time
#endif
#define STEDC_MAXIT 100 // steps of the secular iteration at most: reaching it is an error
#define STEDC_SWEEPS 30 // Jacobi sweeps of a leaf at most: reaching it is an error

namespace {

constexpr int ST = 256;              // threads of the memory-bound kernels
constexpr int SS = STEDC_STRIP;
constexpr double EPSL = 0x1p-53;     // dlamch('Epsilon')
static_assert(STEDC_LEAF == 32, "k_stedc_leaf is written for 32 x 32 blocks");
static_assert(SS % 64 == 0, "STEDC_STRIP is a multiple of the GEMM's tile");

double g_stats[8]; // the last hb_eig_tridiagonal's seconds: leaves, gather + scan, rotations + secular + vectors, U + GEMM, copies + ordering; [5] GEMM flops

// ---- leaves ------------------------------------------------------------------------------------------------------------------------------
// pair `t` (0 .. 15) of step `step` (0 .. 30) of the round-robin order over 32 indices
__device__ __forceinline__ void rr_pair(int step, int t, int *p, int *q)
{
    int a, b;
    if (t == 0) {
        a = 31;
        b = step;
    } else {
        a = (step + t) % 31;
        b = (step - t + 31) % 31;
    }
    *p = min(a, b);
    *q = max(a, b);
}

__global__ __launch_bounds__(64) void k_stedc_leaf(const double *__restrict__ dt, const double *__restrict__ es, const int *__restrict__ leaf_lo,
                                                   const int *__restrict__ leaf_hi, double *__restrict__ Z, int64_t ldz, double *__restrict__ lam,
                                                   int *__restrict__ status)
{
    __shared__ double A[32][33], V[32][33], rc[16], rs[16], rt[16], rapq[16], rapp[16], raqq[16];
    __shared__ int ron[16];
    __shared__ double thr_s;
    const int lane = threadIdx.x, lo = leaf_lo[blockIdx.x], s = leaf_hi[blockIdx.x] - lo;
    for (int x = lane; x < 1024; x += 64) {
        A[x >> 5][x & 31] = 0.0;
        V[x >> 5][x & 31] = (x >> 5) == (x & 31) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (lane < s) A[lane][lane] = dt[lo + lane];
    if (lane < s - 1) A[lane][lane + 1] = A[lane + 1][lane] = es[lo + lane];
    __syncthreads();
    if (lane == 0) {
        double mx = 0.0;
        for (int i = 0; i < s; i++) mx = fmax(mx, fmax(fabs(A[i][i]), i + 1 < s ? fabs(A[i][i + 1]) : 0.0));
        thr_s = EPSL * mx / 32.0;
    }
    __syncthreads();
    const double thr = thr_s;
    bool done = false;
    for (int sweep = 0; sweep < STEDC_SWEEPS && !done; sweep++) {
        int rotated = 0;
        for (int step = 0; step < 31; step++) {
            int on = 0;
            if (lane < 16) {
                int p, q;
                rr_pair(step, lane, &p, &q);
                const double apq = A[p][q];
                on = fabs(apq) > thr;
                double c = 1.0, sn = 0.0, t = 0.0;
                if (on) {
                    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                    // c = 1 - h with h = t^2 / (r (1 + r)), r = sqrt(1 + t^2): 1 / r would inherit the rounding of r on the coarse grid above 1, which
                    // for small t falls just below a tie and always goes one way — half an eps of growth in c^2 + s^2 per rotation, some 25 eps in a
                    // column's norm over the ~200 rotations it sees. h is small and has no such grid
                    t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
                    const double r = sqrt(fma(t, t, 1.0));
                    c = 1.0 - t * t / (r * (1.0 + r));
                    sn = t * c;
                }
                rc[lane] = c;
                rs[lane] = sn;
                rt[lane] = t;
                rapq[lane] = apq;
                rapp[lane] = A[p][p];
                raqq[lane] = A[q][q];
                ron[lane] = on;
            }
            if (!__syncthreads_or(on)) continue;
            rotated = 1;
            for (int x = lane; x < 512; x += 64) { // the columns p, q of A and of V
                const int pr = x >> 5, r = x & 31;
                int p, q;
                rr_pair(step, pr, &p, &q);
                const double c = rc[pr], sn = rs[pr];
                const double a = A[r][p], b = A[r][q], va = V[r][p], vb = V[r][q];
                A[r][p] = c * a - sn * b;
                A[r][q] = sn * a + c * b;
                V[r][p] = c * va - sn * vb;
                V[r][q] = sn * va + c * vb;
            }
            __syncthreads();
            for (int x = lane; x < 512; x += 64) { // the rows p, q of A
                const int pr = x >> 5, cc = x & 31;
                int p, q;
                rr_pair(step, pr, &p, &q);
                const double c = rc[pr], sn = rs[pr];
                const double a = A[p][cc], b = A[q][cc];
                A[p][cc] = c * a - sn * b;
                A[q][cc] = sn * a + c * b;
            }
            __syncthreads();
            if (lane < 16 && ron[lane]) {
                int p, q;
                rr_pair(step, lane, &p, &q);
                // the diagonal by the rotation's own formula, from the values before it; the rotated pair is zero by construction
                A[p][p] = rapp[lane] - rt[lane] * rapq[lane];
                A[q][q] = raqq[lane] + rt[lane] * rapq[lane];
                A[p][q] = 0.0;
                A[q][p] = 0.0;
            }
            __syncthreads();
        }
        done = !rotated;
    }
    if (!done && lane == 0) status[0] = 1;
    if (lane < s) lam[lo + lane] = A[lane][lane];
    for (int x = lane; x < 1024; x += 64) {
        const int r = x & 31, c = x >> 5;
        if (r < s && c < s) Z[(int64_t)(lo + c) * ldz + lo + r] = V[r][c];
    }
}

// ---- merges ------------------------------------------------------------------------------------------------------------------------------
struct merge_dev { // one merge of the level, as the kernels read it
    int lo, mid, hi, kk, nt, nb, rot0, rot1;
    double rho, sign;
};

__global__ __launch_bounds__(ST) void k_stedc_gather(const double *__restrict__ Z, int64_t ldz, int n, const int *__restrict__ mcol,
                                                     const merge_dev *__restrict__ M, double *__restrict__ zraw)
{
    const int p = blockIdx.x * ST + threadIdx.x;
    if (p >= n) return;
    const int m = mcol[p];
    if (m < 0) return;
    const int mid = M[m].mid;
    zraw[p] = p < mid ? Z[(int64_t)p * ldz + mid - 1] : M[m].sign * Z[(int64_t)p * ldz + mid];
}

// x' = c x + s y, y' = c y - s x (drot) on the columns pj, nj over the merge's rows; a thread keeps its rows through the whole list
__global__ __launch_bounds__(ST) void k_stedc_rot(double *__restrict__ Z, int64_t ldz, const merge_dev *__restrict__ M, const int *__restrict__ rot_pj,
                                                  const int *__restrict__ rot_nj, const double *__restrict__ rot_c, const double *__restrict__ rot_s)
{
    const merge_dev mg = M[blockIdx.x];
    for (int r = mg.rot0; r < mg.rot1; r++) {
        double *x = Z + (int64_t)rot_pj[r] * ldz, *y = Z + (int64_t)rot_nj[r] * ldz;
        const double c = rot_c[r], s = rot_s[r];
        for (int i = mg.lo + threadIdx.x; i < mg.hi; i += ST) {
            const double a = x[i], b = y[i];
            x[i] = c * a + s * b;
            y[i] = c * b - s * a;
        }
    }
}

// the secular function 1 / rho + sum_j z_j^2 / (d_j - x) at x = d[org] + tau, the lower poles 0 .. pa from the far end, the upper kk - 1 .. pb too
struct sec_eval {
    double w, dpsi, dphi, err, da, db;
};
__device__ __forceinline__ sec_eval secular_at(const double *__restrict__ dl, const double *__restrict__ zl, int kk, int pa, int pb, int org, double tau,
                                               double rhoinv)
{
    const double dorg = dl[org];
    double psi = 0.0, dpsi = 0.0, phi = 0.0, dphi = 0.0, mag = 0.0;
    for (int j = 0; j <= pa; j++) {
        const double z = zl[j], t = z / ((dl[j] - dorg) - tau), term = z * t;
        psi += term;
        dpsi += t * t;
        mag += fabs(term);
    }
    for (int j = kk - 1; j >= pb; j--) {
        const double z = zl[j], t = z / ((dl[j] - dorg) - tau), term = z * t;
        phi += term;
        dphi += t * t;
        mag += fabs(term);
    }
    sec_eval r;
    r.w = rhoinv + psi + phi;
    r.dpsi = dpsi;
    r.dphi = dphi;
    r.err = 8.0 * mag + 2.0 * rhoinv + fabs(tau) * (dpsi + dphi);
    r.da = (dl[pa] - dorg) - tau;
    r.db = (dl[pb] - dorg) - tau;
    return r;
}

// a point strictly inside the bracket, which never straddles zero: geometric where the ends differ by more than 16, a pole's end (0) left quickly
__device__ __forceinline__ double sec_bisect(double lo, double hi)
{
    const bool neg = hi <= 0.0;
    double a = neg ? -hi : lo, b = neg ? -lo : hi, m;
    if (a == 0.0) m = b * 0x1p-10;
    else if (b > 16.0 * a) m = sqrt(a) * sqrt(b);
    else m = a + 0.5 * (b - a);
    return neg ? -m : m;
}

__global__ __launch_bounds__(64) void k_stedc_secular(int n, const int *__restrict__ mcol, const merge_dev *__restrict__ M, const double *__restrict__ dlv,
                                                      const double *__restrict__ zlv, int *__restrict__ orgv, double *__restrict__ tauv,
                                                      int *__restrict__ status)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    const int m = mcol[p];
    if (m < 0) return;
    const int lo = M[m].lo, kk = M[m].kk, i = p - lo;
    if (i >= kk) return;
    const double *dl = dlv + lo, *zl = zlv + lo;
    const double rho = M[m].rho, rhoinv = 1.0 / rho;
    if (kk == 1) {
        orgv[p] = lo;
        tauv[p] = rho * zl[0] * zl[0];
        return;
    }
    const bool last = i == kk - 1;
    const int pa = last ? i - 1 : i, pb = pa + 1;
    int org = i;
    double blo = 0.0, bhi, tau;
    if (last) {
        double s = 0.0;
        for (int j = 0; j < kk; j++) s += zl[j] * zl[j];
        bhi = rho * s;
        tau = bhi;
    } else {
        const double half = 0.5 * (dl[i + 1] - dl[i]);
        if (secular_at(dl, zl, kk, pa, pb, i, half, rhoinv).w >= 0.0) {
            bhi = half;
            tau = half;
        } else {
            org = i + 1;
            blo = -half;
            bhi = 0.0;
            tau = -half;
        }
    }
    bool ok = false;
    for (int it = 0; it < STEDC_MAXIT; it++) {
        const sec_eval f = secular_at(dl, zl, kk, pa, pb, org, tau, rhoinv);
        if (fabs(f.w) <= EPSL * f.err) {
            ok = true;
            break;
        }
        if (f.w < 0.0) blo = tau;
        else bhi = tau;
        const double mid = sec_bisect(blo, bhi);
        if (!(blo < mid && mid < bhi)) { // no number between the bracket's ends: the root to working precision, at the end that is no pole
            tau = blo == 0.0 ? bhi : bhi == 0.0 ? blo : tau;
            ok = true;
            break;
        }
        // both roots of c eta^2 - a eta + b = 0, the osculating rational with the poles pa, pb: at most one lies inside the bracket
        const double dw = f.dpsi + f.dphi;
        const double c = f.w - f.da * f.dpsi - f.db * f.dphi, a = (f.da + f.db) * f.w - f.da * f.db * dw, b = f.da * f.db * f.w;
        double r1, r2;
        if (c == 0.0) r1 = r2 = b / a;
        else {
            const double sq = sqrt(fabs(a * a - 4.0 * b * c));
            if (a >= 0.0) {
                r1 = (a + sq) / (2.0 * c);
                r2 = 2.0 * b / (a + sq);
            } else {
                r1 = (a - sq) / (2.0 * c);
                r2 = 2.0 * b / (a - sq);
            }
        }
        double nt = mid;
        if (blo < tau + r1 && tau + r1 < bhi) nt = tau + r1;
        else if (blo < tau + r2 && tau + r2 < bhi) nt = tau + r2;
        tau = nt;
    }
    if (!ok) status[1] = 1;
    orgv[p] = lo + org;
    tauv[p] = tau;
}

// zhat_j = sign(z_j) sqrt(-(d_j - x_j) prod_{i != j} (d_j - x_i) / (d_j - d_i)), the roots in index order, one ratio at a time (dlaed3)
__global__ __launch_bounds__(64) void k_stedc_lowner(int n, const int *__restrict__ mcol, const merge_dev *__restrict__ M, const double *__restrict__ dlv,
                                                     const double *__restrict__ zlv, const int *__restrict__ orgv, const double *__restrict__ tauv,
                                                     double *__restrict__ zh)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    const int m = mcol[p];
    if (m < 0) return;
    const int lo = M[m].lo, kk = M[m].kk, j = p - lo;
    if (j >= kk) return;
    const double dj = dlv[p];
    double w = (dj - dlv[orgv[p]]) - tauv[p];
    for (int i = 0; i < kk; i++) {
        if (i == j) continue;
        w *= ((dj - dlv[orgv[lo + i]]) - tauv[lo + i]) / (dj - dlv[lo + i]);
    }
    zh[p] = copysign(sqrt(-w), zlv[p]);
}

// root i: 1 / ||(zhat_j / ((d_j - d_org) - tau))_j||, the poles in index order; its eigenvalue d_org + tau
__global__ __launch_bounds__(64) void k_stedc_norm(int n, const int *__restrict__ mcol, const merge_dev *__restrict__ M, const double *__restrict__ dlv,
                                                   const int *__restrict__ orgv, const double *__restrict__ tauv, const double *__restrict__ zh,
                                                   double *__restrict__ inorm, double *__restrict__ lamnew)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    const int m = mcol[p];
    if (m < 0) return;
    const int lo = M[m].lo, kk = M[m].kk;
    if (p - lo >= kk) return;
    const double dorg = dlv[orgv[p]], tau = tauv[p];
    double s = 0.0;
    for (int j = 0; j < kk; j++) {
        const double u = zh[lo + j] / ((dlv[lo + j] - dorg) - tau);
        s = fma(u, u, s);
    }
    inorm[p] = 1.0 / sqrt(s);
    lamnew[p] = dorg + tau;
}

// Ut[(lo + j) * SS + cc] = U[j][strip * SS + cc]: a workgroup per pole, a thread per root of the strip; zero past the merge's last root
__global__ __launch_bounds__(SS) void k_stedc_ubuild(int strip, const int *__restrict__ mcol, const merge_dev *__restrict__ M, const double *__restrict__ dlv,
                                                     const int *__restrict__ orgv, const double *__restrict__ tauv, const double *__restrict__ zh,
                                                     const double *__restrict__ inorm, double *__restrict__ Ut)
{
    const int p = blockIdx.x, m = mcol[p];
    if (m < 0) return;
    const int lo = M[m].lo, kk = M[m].kk;
    if (p - lo >= kk || strip * SS >= kk) return;
    const int i = strip * SS + threadIdx.x;
    double u = 0.0;
    if (i < kk) u = zh[p] * inorm[lo + i] / ((dlv[p] - dlv[orgv[lo + i]]) - tauv[lo + i]);
    Ut[(int64_t)p * SS + threadIdx.x] = u;
}

// Znew[i][lo + c] = sum_t Zold[i][src[t]] U[list[t]][c] for the rows i of one child and the roots c of the strip: 64 x 64 tiles, four waves of
// 32 x 32 (hb_mma.hpp: mfma_f64 and its layout), the list in its order, four entries per MFMA. blockIdx.y = 2 * merge + child; blockIdx.x = 4-column-tile strips by row tiles. Rows past
// the child's last are read from its last row and not stored; list entries past its end enter as zeros on both sides.
__global__ __launch_bounds__(256) void k_stedc_gemm(int strip, const merge_dev *__restrict__ M, const int *__restrict__ tlist, const int *__restrict__ blist,
                                                    const int *__restrict__ tsrc, const int *__restrict__ bsrc, const double *__restrict__ Zold,
                                                    double *__restrict__ Znew, int64_t ldz, const double *__restrict__ Ut)
{
    const merge_dev mg = M[blockIdx.y >> 1];
    const int child = blockIdx.y & 1, tr = blockIdx.x / (SS / 64), tc = blockIdx.x % (SS / 64);
    const int r0 = child ? mg.mid : mg.lo, r1 = child ? mg.hi : mg.mid;
    if (strip * SS + tc * 64 >= mg.kk || r0 + tr * 64 >= r1) return;
    const int *list = (child ? blist : tlist) + mg.lo, *src = (child ? bsrc : tsrc) + mg.lo; // list[t]: the pole's index, src[t]: its column of Zold
    const int L = child ? mg.nb : mg.nt;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wr = wave >> 1, wc = wave & 1, lr = lane & 15, q = lane >> 4;
    const int i0 = r0 + tr * 64 + wr * 32, cb = tc * 64 + wc * 32;
    v4d acc[2][2];
    mma_f64_zero(acc);
    const int ra = min(i0 + lr, r1 - 1), rb = min(i0 + 16 + lr, r1 - 1);
    for (int s4 = 0; s4 < L; s4 += 4) {
        const int t = s4 + q;
        double zi[2] = {0.0, 0.0}, uj[2] = {0.0, 0.0};
        if (t < L) {
            const int j = list[t];
            const double *zc = Zold + (int64_t)src[t] * ldz, *ur = Ut + (int64_t)(mg.lo + j) * SS + cb + lr;
            zi[0] = zc[ra];
            zi[1] = zc[rb];
            uj[0] = ur[0];
            uj[1] = ur[16];
        }
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++) acc[a][b] = mfma_f64(uj[b], zi[a], acc[a][b]); // D[c][i] += U[j][c] Z[i][j]
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = i0 + mma_f64_col(a, lane), c = strip * SS + cb + mma_f64_row(b, r, lane);
                if (i < r1 && c < mg.kk) Znew[(int64_t)(mg.lo + c) * ldz + i] = acc[a][b][r];
            }
}

// column cp[4 b] of Zold to column cp[4 b + 1] of Znew over the rows cp[4 b + 2] .. cp[4 b + 3] - 1
__global__ __launch_bounds__(ST) void k_stedc_copy(const int *__restrict__ cp, const double *__restrict__ Zold, double *__restrict__ Znew, int64_t ldz)
{
    const int *c = cp + 4 * (int64_t)blockIdx.x;
    const double *x = Zold + (int64_t)c[0] * ldz;
    double *y = Znew + (int64_t)c[1] * ldz;
    for (int i = c[2] + threadIdx.x; i < c[3]; i += ST) y[i] = x[i];
}

// column j of Znew = column order[j] of Zold, rows 0 .. n - 1
__global__ __launch_bounds__(ST) void k_stedc_permute(const int *__restrict__ order, int n, const double *__restrict__ Zold, double *__restrict__ Znew, int64_t ldz)
{
    const double *x = Zold + (int64_t)order[blockIdx.x] * ldz;
    double *y = Znew + (int64_t)blockIdx.x * ldz;
    for (int i = threadIdx.x; i < n; i += ST) y[i] = x[i];
}

__global__ __launch_bounds__(ST) void k_stedc_identity(double *__restrict__ Z, int64_t ldz, int n)
{
    const int i = blockIdx.x * ST + threadIdx.x;
    if (i < n) Z[(int64_t)i * ldz + i] = 1.0;
}

inline unsigned blocks(int64_t count, int per) { return (unsigned)std::max<int64_t>(1, (count + per - 1) / per); }

// dlaed2's scan on one merge (host, O(k log k)): what[lo .. hi) positions are relative to lo
struct scan_out {
    std::vector<int> keep, defl, typ;
    std::vector<double> d, z;
    std::vector<int> rot_pj, rot_nj;
    std::vector<double> rot_c, rot_s;
    double rho = 0.0;
};

void deflate(const double *lam, const double *zraw, int k, int k1, double rho0, scan_out &o)
{
    o.rho = 2.0 * rho0;
    o.d.assign(lam, lam + k);
    o.z.resize(k);
    o.typ.resize(k);
    double dmax = 0.0, zmax = 0.0;
    for (int j = 0; j < k; j++) {
        o.z[j] = zraw[j] / std::sqrt(2.0);
        o.typ[j] = j < k1 ? 1 : 3;
        dmax = std::max(dmax, std::fabs(o.d[j]));
        zmax = std::max(zmax, std::fabs(o.z[j]));
    }
    std::vector<int> order(k);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return o.d[a] < o.d[b]; });
    const double tol = 8.0 * EPSL * std::max(dmax, zmax);
    if (o.rho * zmax <= tol) {
        o.defl = order;
        return;
    }
    int pj = -1;
    for (int j : order) {
        if (o.rho * std::fabs(o.z[j]) <= tol) {
            o.defl.push_back(j);
            continue;
        }
        if (pj < 0) {
            pj = j;
            continue;
        }
        double s = o.z[pj], c = o.z[j];
        const double tau = std::hypot(c, s), t = o.d[j] - o.d[pj];
        c /= tau;
        s = -s / tau;
        if (std::fabs(t * c * s) <= tol) {
            o.z[j] = tau;
            o.z[pj] = 0.0;
            o.rot_pj.push_back(pj);
            o.rot_nj.push_back(j);
            o.rot_c.push_back(c);
            o.rot_s.push_back(s);
            if (o.typ[pj] != o.typ[j]) o.typ[j] = 2;
            const double t2 = o.d[pj] * c * c + o.d[j] * s * s;
            o.d[j] = o.d[pj] * s * s + o.d[j] * c * c;
            o.d[pj] = t2;
            o.defl.push_back(pj);
        } else
            o.keep.push_back(pj);
        pj = j;
    }
    o.keep.push_back(pj);
}

template <typename T> int to_device(T *dst, const std::vector<T> &v, hipStream_t s)
{
    if (!v.empty()) HB_HIP(hipMemcpyAsync(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, s));
    return HB_OK;
}

// Z and W: ldz x ldz, zeroed. On return *Zfinal is the one of the two that holds the vectors.
int stedc_run(const double *d, const double *e, int n, double *w, double *Z, double *W, int64_t ldz, hipStream_t st, double **Zfinal)
{
    hb_bufs mem;
    auto t0 = hb_clk::now();
    for (double &x : g_stats) x = 0.0;
    double sigma = 0.0;
    for (int i = 0; i < n; i++) sigma = std::max(sigma, std::max(std::fabs(d[i]), i + 1 < n ? std::fabs(e[i]) : 0.0));
    *Zfinal = Z;
    if (sigma == 0.0) {
        for (int i = 0; i < n; i++) w[i] = 0.0;
        hipLaunchKernelGGL(k_stedc_identity, dim3(blocks(n, ST)), dim3(ST), 0, st, Z, ldz, n);
        HB_HIP(hipGetLastError());
        HB_HIP(hipStreamSynchronize(st));
        return HB_OK;
    }
    std::vector<double> ds(n), es(n, 0.0), dt;
    for (int i = 0; i < n; i++) ds[i] = d[i] / sigma;
    for (int i = 0; i + 1 < n; i++) es[i] = e[i] / sigma;
    std::vector<int32_t> splits;
    std::vector<char> cut(n + 1, 0); // cut[i]: a part starts at row i
    cut[0] = cut[n] = 1;
    for (int i = 0; i + 1 < n; i++)
        if (std::fabs(es[i]) <= EPSL * std::sqrt(std::fabs(ds[i])) * std::sqrt(std::fabs(ds[i + 1]))) {
            splits.push_back(i);
            cut[i + 1] = 1;
        }
    const hb_stedc_tree tree = hb_stedc_tree_of(n, splits.data(), (int32_t)splits.size());
    dt = ds;
    for (const hb_stedc_merge &m : tree.merges) {
        const double rho = std::fabs(es[m.mid - 1]);
        dt[m.mid - 1] -= rho;
        dt[m.mid] -= rho;
    }
    const int nleaf = (int)tree.leaf_lo.size();
    // device vectors
    double *g_dt, *g_es, *g_lam, *g_zraw, *g_dl, *g_zl, *g_tau, *g_zh, *g_inorm, *g_rc, *g_rs, *g_Ut = nullptr;
    int *g_llo, *g_lhi, *g_status, *g_mcol, *g_org, *g_tl, *g_bl, *g_ts, *g_bs, *g_rpj, *g_rnj, *g_cp, *g_order;
    merge_dev *g_M;
    HB_TRY(mem.get(&g_dt, n)); HB_TRY(mem.get(&g_es, n)); HB_TRY(mem.zeroed(&g_lam, n, st)); HB_TRY(mem.zeroed(&g_zraw, n, st));
    HB_TRY(mem.zeroed(&g_dl, n, st)); HB_TRY(mem.zeroed(&g_zl, n, st)); HB_TRY(mem.zeroed(&g_tau, n, st)); HB_TRY(mem.zeroed(&g_zh, n, st));
    HB_TRY(mem.zeroed(&g_inorm, n, st)); HB_TRY(mem.get(&g_rc, n)); HB_TRY(mem.get(&g_rs, n));
    HB_TRY(mem.get(&g_llo, nleaf)); HB_TRY(mem.get(&g_lhi, nleaf)); HB_TRY(mem.zeroed(&g_status, 2, st)); HB_TRY(mem.get(&g_mcol, n));
    HB_TRY(mem.zeroed(&g_org, n, st)); HB_TRY(mem.get(&g_tl, n)); HB_TRY(mem.get(&g_bl, n)); HB_TRY(mem.get(&g_ts, n)); HB_TRY(mem.get(&g_bs, n)); HB_TRY(mem.get(&g_rpj, n));
    HB_TRY(mem.get(&g_rnj, n)); HB_TRY(mem.get(&g_cp, (size_t)4 * n)); HB_TRY(mem.get(&g_order, n));
    HB_TRY(mem.get(&g_M, std::max<size_t>(1, tree.merges.size())));
    const bool any_merge = !tree.merges.empty();
    if (any_merge) HB_TRY(mem.big(&g_Ut, (size_t)n * SS, "hb_eig_tridiagonal", "the strip of U of the " + hb_dims(n) + " eigenvector matrix"));
    HB_HIP(hipMemcpyAsync(g_dt, dt.data(), sizeof(double) * n, hipMemcpyHostToDevice, st));
    HB_HIP(hipMemcpyAsync(g_es, es.data(), sizeof(double) * n, hipMemcpyHostToDevice, st));
    {
        std::vector<int> llo(tree.leaf_lo.begin(), tree.leaf_lo.end()), lhi(tree.leaf_hi.begin(), tree.leaf_hi.end());
        HB_TRY(to_device(g_llo, llo, st));
        HB_TRY(to_device(g_lhi, lhi, st));
        hipLaunchKernelGGL(k_stedc_leaf, dim3((unsigned)nleaf), dim3(64), 0, st, g_dt, g_es, g_llo, g_lhi, Z, ldz, g_lam, g_status);
        HB_HIP(hipGetLastError());
    }
    std::vector<double> lam(n), zraw(n), lamnew(n);
    int status[2] = {0, 0};
    HB_HIP(hipMemcpyAsync(lam.data(), g_lam, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HB_HIP(hipMemcpyAsync(status, g_status, sizeof status, hipMemcpyDeviceToHost, st));
    HB_HIP(hipStreamSynchronize(st));
    if (status[0]) return hb_fail(HB_ERR_HIP, "hb_eig_tridiagonal: a leaf's Jacobi sweeps did not converge in " + std::to_string(STEDC_SWEEPS) + " sweeps");
    g_stats[0] = hb_since(t0);
    std::vector<int> blo(n), bhi(n); // the finished node that holds each column
    for (int l = 0; l < nleaf; l++)
        for (int p = tree.leaf_lo[l]; p < tree.leaf_hi[l]; p++) {
            blo[p] = tree.leaf_lo[l];
            bhi[p] = tree.leaf_hi[l];
        }
    double *Zold = Z, *Znew = W;
    for (int level = 1; level <= tree.levels; level++) {
        auto t1 = hb_clk::now();
        std::vector<merge_dev> M;
        std::vector<int> mcol(n, -1);
        for (const hb_stedc_merge &m : tree.merges)
            if (m.level == level) {
                merge_dev g{};
                g.lo = m.lo, g.mid = m.mid, g.hi = m.hi;
                g.rho = std::fabs(es[m.mid - 1]);
                g.sign = es[m.mid - 1] >= 0.0 ? 1.0 : -1.0;
                for (int p = m.lo; p < m.hi; p++) mcol[p] = (int)M.size();
                M.push_back(g);
            }
        const int nm = (int)M.size();
        HB_TRY(to_device(g_mcol, mcol, st));
        HB_TRY(to_device(g_M, M, st));
        hipLaunchKernelGGL(k_stedc_gather, dim3(blocks(n, ST)), dim3(ST), 0, st, Zold, ldz, n, g_mcol, g_M, g_zraw);
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(zraw.data(), g_zraw, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HB_HIP(hipStreamSynchronize(st));
        std::vector<double> dl(n, 0.0), zl(n, 0.0), rc, rs;
        std::vector<int> tl(n, 0), bl(n, 0), ts(n, 0), bs(n, 0), rpj, rnj, cp;
        int maxkk = 0, maxrows = 0;
        std::vector<std::vector<double>> dnew(nm);
        for (int mi = 0; mi < nm; mi++) {
            merge_dev &g = M[mi];
            const int lo = g.lo, k = g.hi - g.lo;
            scan_out o;
            deflate(lam.data() + lo, zraw.data() + lo, k, g.mid - lo, g.rho, o);
            g.rho = o.rho;
            g.kk = (int)o.keep.size();
            g.rot0 = (int)rpj.size();
            for (size_t r = 0; r < o.rot_pj.size(); r++) {
                rpj.push_back(lo + o.rot_pj[r]);
                rnj.push_back(lo + o.rot_nj[r]);
                rc.push_back(o.rot_c[r]);
                rs.push_back(o.rot_s[r]);
            }
            g.rot1 = (int)rpj.size();
            g.nt = g.nb = 0;
            for (int j = 0; j < g.kk; j++) {
                const int pos = o.keep[j];
                dl[lo + j] = o.d[pos];
                zl[lo + j] = o.z[pos];
                if (o.typ[pos] <= 2) {
                    tl[lo + g.nt] = j;
                    ts[lo + g.nt++] = lo + pos;
                }
                if (o.typ[pos] >= 2) {
                    bl[lo + g.nb] = j;
                    bs[lo + g.nb++] = lo + pos;
                }
            }
            dnew[mi].resize(k);
            for (size_t t = 0; t < o.defl.size(); t++) {
                const int pos = o.defl[t], dst = lo + g.kk + (int)t;
                cp.insert(cp.end(), {lo + pos, dst, lo, g.hi});
                dnew[mi][g.kk + t] = o.d[pos];
            }
            maxkk = std::max(maxkk, g.kk);
            maxrows = std::max(maxrows, std::max(g.mid - g.lo, g.hi - g.mid));
            g_stats[5] += 2.0 * (double)g.kk * ((double)(g.mid - g.lo) * g.nt + (double)(g.hi - g.mid) * g.nb);
        }
        for (int p = 0; p < n; p++) // a finished node that waits for a later level moves to the other buffer as it is
            if (mcol[p] < 0) cp.insert(cp.end(), {p, p, blo[p], bhi[p]});
        HB_TRY(to_device(g_M, M, st));
        HB_TRY(to_device(g_dl, dl, st)); HB_TRY(to_device(g_zl, zl, st)); HB_TRY(to_device(g_tl, tl, st)); HB_TRY(to_device(g_bl, bl, st));
        HB_TRY(to_device(g_ts, ts, st)); HB_TRY(to_device(g_bs, bs, st)); HB_TRY(to_device(g_rpj, rpj, st)); HB_TRY(to_device(g_rnj, rnj, st)); HB_TRY(to_device(g_rc, rc, st));
        HB_TRY(to_device(g_rs, rs, st)); HB_TRY(to_device(g_cp, cp, st));
        g_stats[1] += hb_since(t1);
        t1 = hb_clk::now();
        if (!rpj.empty()) hipLaunchKernelGGL(k_stedc_rot, dim3((unsigned)nm), dim3(ST), 0, st, Zold, ldz, g_M, g_rpj, g_rnj, g_rc, g_rs);
        if (maxkk > 0) {
            hipLaunchKernelGGL(k_stedc_secular, dim3(blocks(n, 64)), dim3(64), 0, st, n, g_mcol, g_M, g_dl, g_zl, g_org, g_tau, g_status);
            hipLaunchKernelGGL(k_stedc_lowner, dim3(blocks(n, 64)), dim3(64), 0, st, n, g_mcol, g_M, g_dl, g_zl, g_org, g_tau, g_zh);
            hipLaunchKernelGGL(k_stedc_norm, dim3(blocks(n, 64)), dim3(64), 0, st, n, g_mcol, g_M, g_dl, g_org, g_tau, g_zh, g_inorm, g_lam);
        }
        HB_HIP(hipGetLastError());
        HB_HIP(hipMemcpyAsync(lamnew.data(), g_lam, sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HB_HIP(hipMemcpyAsync(status, g_status, sizeof status, hipMemcpyDeviceToHost, st));
        HB_HIP(hipStreamSynchronize(st));
        if (status[1])
            return hb_fail(HB_ERR_HIP, "hb_eig_tridiagonal: the secular equation's iteration did not converge in " + std::to_string(STEDC_MAXIT) + " steps");
        g_stats[2] += hb_since(t1);
        t1 = hb_clk::now();
        const int nstrip = (maxkk + SS - 1) / SS;
        for (int s = 0; s < nstrip; s++) {
            hipLaunchKernelGGL(k_stedc_ubuild, dim3((unsigned)n), dim3(SS), 0, st, s, g_mcol, g_M, g_dl, g_org, g_tau, g_zh, g_inorm, g_Ut);
            hipLaunchKernelGGL(k_stedc_gemm, dim3((unsigned)((maxrows + 63) / 64 * (SS / 64)), (unsigned)(2 * nm)), dim3(256), 0, st, s, g_M, g_tl, g_bl, g_ts, g_bs,
                               Zold, Znew, ldz, g_Ut);
        }
        HB_HIP(hipGetLastError());
        HB_HIP(hipStreamSynchronize(st));
        g_stats[3] += hb_since(t1);
        t1 = hb_clk::now();
        if (!cp.empty()) hipLaunchKernelGGL(k_stedc_copy, dim3((unsigned)(cp.size() / 4)), dim3(ST), 0, st, g_cp, Zold, Znew, ldz);
        HB_HIP(hipGetLastError());
        HB_HIP(hipStreamSynchronize(st));
        g_stats[4] += hb_since(t1);
        for (int mi = 0; mi < nm; mi++) {
            const merge_dev &g = M[mi];
            for (int p = g.lo; p < g.hi; p++) {
                lam[p] = p - g.lo < g.kk ? lamnew[p] : dnew[mi][p - g.lo];
                blo[p] = g.lo;
                bhi[p] = g.hi;
            }
        }
        std::swap(Zold, Znew);
    }
    // unscale (a 1 x 1 part's eigenvalue is its entry, untouched by the scaling) and order
    auto t1 = hb_clk::now();
    std::vector<double> wu(n);
    for (int p = 0; p < n; p++) wu[p] = (cut[p] && cut[p + 1]) ? d[p] : lam[p] * sigma;
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return wu[a] < wu[b]; });
    for (int j = 0; j < n; j++) w[j] = wu[order[j]];
    HB_TRY(to_device(g_order, order, st));
    hipLaunchKernelGGL(k_stedc_permute, dim3((unsigned)n), dim3(ST), 0, st, g_order, n, Zold, Znew, ldz);
    HB_HIP(hipGetLastError());
    HB_HIP(hipStreamSynchronize(st));
    g_stats[4] += hb_since(t1);
    *Zfinal = Znew;
    return HB_OK;
}

} // namespace

extern "C" {

// the plan of hb_stedcplan.hpp, for the tests: leaves (lo, hi), merges (lo, mid, hi, level) children before parents. cap: the arrays' lengths.
int hb_stedc_plan(int32_t n, const int32_t *splits, int32_t nsplit, int32_t cap, int32_t *leaf_lo, int32_t *leaf_hi, int32_t *nleaf, int32_t *merge_lo,
                  int32_t *merge_mid, int32_t *merge_hi, int32_t *merge_level, int32_t *nmerge, int32_t *levels, int32_t *leaf_rows)
{
    if (!leaf_lo || !leaf_hi || !nleaf || !merge_lo || !merge_mid || !merge_hi || !merge_level || !nmerge || !levels || (nsplit > 0 && !splits))
        return hb_fail(HB_ERR_INVALID, "hb_stedc_plan: null argument");
    if (n < 1 || nsplit < 0) return hb_fail(HB_ERR_INVALID, "hb_stedc_plan: n < 1 or a negative number of split points");
    for (int32_t s = 0; s < nsplit; s++)
        if (splits[s] < 0 || splits[s] >= n - 1 || (s > 0 && splits[s] <= splits[s - 1]))
            return hb_fail(HB_ERR_INVALID, "hb_stedc_plan: the split points must be ascending and inside [0, n - 1)");
    const hb_stedc_tree t = hb_stedc_tree_of(n, splits, nsplit);
    if ((int64_t)t.leaf_lo.size() > cap || (int64_t)t.merges.size() > cap) return hb_fail(HB_ERR_INVALID, "hb_stedc_plan: the arrays are too short for the plan");
    *nleaf = (int32_t)t.leaf_lo.size();
    *nmerge = (int32_t)t.merges.size();
    *levels = t.levels;
    if (leaf_rows) *leaf_rows = STEDC_LEAF;
    for (size_t i = 0; i < t.leaf_lo.size(); i++) {
        leaf_lo[i] = t.leaf_lo[i];
        leaf_hi[i] = t.leaf_hi[i];
    }
    for (size_t i = 0; i < t.merges.size(); i++) {
        merge_lo[i] = t.merges[i].lo;
        merge_mid[i] = t.merges[i].mid;
        merge_hi[i] = t.merges[i].hi;
        merge_level[i] = t.merges[i].level;
    }
    return HB_OK;
}

// dstedc on the device: w_host (n, ascending) and Z on the device, column j belonging to w[j], in hb_eig_vectors' layout (*ldz = n rounded up to 64,
// *ldz columns allocated, padding zero); hb_eig_release frees it, or hb_eig_vectors_dev takes it over.
int hb_eig_tridiagonal(const double *d_host, const double *e_host, int32_t n, int32_t device, double *w_host, double **Z_dev, int64_t *ldz)
{
    if (Z_dev) *Z_dev = nullptr;
    if (!d_host || !w_host || !Z_dev || !ldz || (n > 1 && !e_host)) return hb_fail(HB_ERR_INVALID, "hb_eig_tridiagonal: null argument");
    if (n < 1) return hb_fail(HB_ERR_INVALID, "hb_eig_tridiagonal: n < 1");
    for (int i = 0; i < n; i++)
        if (!std::isfinite(d_host[i]) || (i < n - 1 && !std::isfinite(e_host[i])))
            return hb_fail(HB_ERR_INVALID, "hb_eig_tridiagonal: the tridiagonal matrix holds a non-finite value");
    if (hb_device_count() <= 0) return hb_fail(HB_ERR_NO_DEVICE, "no HIP device available: the hibayes GPU engine has no CPU fallback");
    HB_HIP(hipSetDevice(device));
    const int64_t ld = ((int64_t)n + 63) / 64 * 64;
    const size_t bytes = sizeof(double) * (size_t)ld * (size_t)ld;
    hb_bufs mem;
    double *Z = nullptr, *W = nullptr;
    char both[96]; // (the call holds two such matrices: the refusal of either tells the total as well)
    snprintf(both, sizeof both, " (the call needs it and a workspace as large, %.1f GB together)", 2e-9 * (double)bytes);
    HB_TRY(mem.big(&Z, (size_t)ld * (size_t)ld, "hb_eig_tridiagonal", "the " + hb_dims(n) + " eigenvector matrix" + both));
    HB_TRY(mem.big(&W, (size_t)ld * (size_t)ld, "hb_eig_tridiagonal", "the workspace of the " + hb_dims(n) + " eigenvector matrix" + both));
    hipStream_t st = nullptr;
    double *Zf = nullptr;
    auto run = [&]() -> int {
        HB_HIP(hipStreamCreate(&st));
        HB_HIP(hipMemsetAsync(Z, 0, bytes, st));
        HB_HIP(hipMemsetAsync(W, 0, bytes, st));
        return stedc_run(d_host, e_host, n, w_host, Z, W, ld, st, &Zf);
    };
    const int rc = run();
    if (st) {
        (void)hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
    }
    if (rc) return rc;
    mem.release(Zf); // the caller's from here (hb_eig_release, or hb_eig_vectors_dev takes it over); the other of the two goes with this call
    *Z_dev = Zf;
    *ldz = ld;
    return HB_OK;
}

// seconds of the last hb_eig_tridiagonal of this process by phase, for tools/eig_timing.py: [0] leaves, [1] gather and the deflation scan, [2]
// rotations, secular equation and vector work, [3] U strips and GEMM, [4] copies and ordering; [5] the GEMM's floating-point operations
int hb_stedc_stats(double *out, int32_t count)
{
    if (!out || count < 1) return hb_fail(HB_ERR_INVALID, "hb_stedc_stats: null argument");
    for (int i = 0; i < count; i++) out[i] = i < 8 ? g_stats[i] : 0.0;
    return HB_OK;
}

} // extern "C"
