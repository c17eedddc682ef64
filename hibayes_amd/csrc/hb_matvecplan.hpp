// hb_matvecplan.hpp — the shape of one launch of the fixed-point panel mat-vec (precise == 2): which kernel runs, with which template arguments, how
// many stages a tile gets, how many tiles, how much LDS, how many blocks when update and finalize rows ride along. The one statement of it: launch_dotq
// (hb_kernels.hip) describes the launch, asks plan_matvec and applies the answer; hb_ctx_create fills the knobs once. It is the third layer under
// hb_runplan.hpp (which geometry a run takes) and hb_plan.hpp (which chain a sweep runs). No HIP in here: plain g++ -std=c++17, and
// tests/test_host_logic.py prints every plan against tests/golden/matvec_plan_table.json. The constants and LDS formulas of the kernels' stage buffers
// live here because the plan budgets with them and the launch sizes with them; hb_matvec.hpp, hb_dotq2.hpp and hb_update.hpp describe what they mean.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#define HB_ND 7 /* int8 digits of the fixed-point residual: 55 bits + sign */

// ---- the kernels' stage geometry and dynamic LDS ----
// k_dotq (hb_matvec.hpp)
#define HBQ_RS 128                       /* rows per stage */
#define HBQ_SLOT 1040
#define HBQ_NX 8                         /* DMA pieces per stage for the genotype tile (8 columns x 128 rows each) */
#define HBQ_XB (HBQ_NX * HBQ_SLOT)
#define HBQ_BUF (HBQ_XB + 1024)          /* + one piece for the 7 digit planes */
#define HBQ_PER (HBQ_NX + 1)
#define HBQ_LDS (2 * HBQ_BUF)
// the dense update rows that ride in a k_dotq launch (hb_update.hpp, update_rows_dense)
#define HBU_SLAB 8448
#define HBU_LDS (HBU_SLAB + 16384)
// k_dotq2<CPL, RS> (hb_dotq2.hpp)
static constexpr int q2_lds(int cpl, int rs) { return 2 * ((64 * cpl / (4096 / rs)) * HBQ_SLOT + ((HB_ND + 1024 / rs - 1) / (1024 / rs)) * 1024); }
// k_dotq2m<CT, G, SC> (hb_dotq2.hpp): 256-individual stages, G of them requested together; G = 0 / 3: the 512-individual stages (3: the conflict-free lane order)
#define Q2M_RS 256
#define Q2M_DSTRIDE 1088
#ifndef Q2M_NBUF
#define Q2M_NBUF 3 /* stage buffers: NBUF - 1 (super-)stages in flight ahead of the one being multiplied (a stage computes in ~0.3 us, a loaded round trip takes ~2) */
#endif
static constexpr int q2m512_lds(bool swz) { return Q2M_NBUF * (8 * (swz ? 1152 : HBQ_SLOT) + 4 * 1024); }
static constexpr int q2m_lds(int ct, int g) { return g == 0 || g == 3 ? q2m512_lds(g == 3) : Q2M_NBUF * g * (ct * HBQ_SLOT + 2 * Q2M_DSTRIDE); }
// k_dotq2r (hb_dotq2.hpp): no dynamic LDS
#define Q2R_RB 4096 /* individuals per row block (64 lanes x 64) */
#define Q2R_CB 4    /* columns per batch */

// ---- the built instantiations of the 2-bit mat-vec: the one list, expanded by hb_kernels.hip into its launch table and by the test into the set every plan must lie in ----
// k_dotq2m<CT, G, SC>: column tiles of 16 per wave, stages requested together (0 / 3: 512-individual stages), one accumulator set per scale or one
#define HB_DOTQ2M_KERNELS(X) X(4, 0, 0) X(4, 0, 1) X(4, 3, 0) X(4, 3, 1) X(16, 1, 0) X(16, 1, 1) X(8, 2, 0) X(8, 2, 1) X(8, 1, 0) X(8, 1, 1) \
    X(4, 2, 0) X(4, 2, 1) X(4, 1, 0) X(4, 1, 1)
// k_dotq2<CPL, RS>: columns per lane, individuals per stage (RS = 128: 6208 bytes of LDS per wave, twice the waves per compute unit)
#define HB_DOTQ2_KERNELS(X) X(2, 512) X(2, 256) X(1, 512) X(1, 128) X(1, 256)

// ---- the knobs (hb_ctx::mv; the environment at hb_ctx_create, the kind also through hb_ctx_set_matvec_kernel) ----
struct hb_matvec_knobs {
    int dotq_tiles = 768;          // tiles per k_dotq launch (HB_DOTQ_TILES): about three waves per compute unit
    bool dotq2_tiles_set = false;  // HB_DOTQ2_TILES given: it then also holds for k_dotq2m, whose own targets and XCD budget (plan_matvec) are skipped
    // tiles per full-width k_dotq2 launch (HB_DOTQ2_TILES): 1568 of seven stages at n = 50k — with two waves per SIMD (k_dotq2 allocates 176 VGPRs for that)
    // 2048 waves are resident, and tiles + update rows + the chain's and k_fwd's compute units must fit; until that cap 2000 -> 1848 tiles of six stages:
    // 296 against 300 sweeps/s
    int dotq2_tiles = 1600;
    int dotq2_cpl = 1, dotq2_rs = 256; // k_dotq2's shape (HB_DOTQ2_CPL, HB_DOTQ2_RS)
    // which kernel computes the panel mat-vec on 2-bit resident genotypes (HB_DOTQ2_KIND / hb_ctx_set_matvec_kernel; all three give the same exact integers):
    // 2 (default since round 5) k_dotq2m, the seven digit planes as a skinny int8 GEMM on the matrix cores — 12.0 us per 3584-column launch isolated; 0 k_dotq2,
    // lane = column through LDS, v_dot4 (22 us: VALU-issue-bound; the default until round 4); 1 k_dotq2r, individuals across the lanes, no LDS, NC columns per tile (26 us)
    int kind = 2, nc = 16; // (nc: HB_DOTQ2_NC)
    // k_dotq2m's shape (HB_Q2M_CT / _G / _SC): column tiles of 16 per wave; stages requested together (1, 2) or 512-individual stages of whole-line DMA pieces
    // (0, the default since round 5: 12.3 against 15.3 us per launch; 3: the same with conflict-free lane order); per-scale accumulators
    int q2m_ct = 4, q2m_g = 0, q2m_sc = 1;
};

// the knobs as the environment sets them (get: getenv, or the test's table)
static inline hb_matvec_knobs matvec_knobs_from_env(const char *(*get)(const char *))
{
    hb_matvec_knobs k;
    if (const char *e = get("HB_DOTQ2_CPL")) k.dotq2_cpl = atoi(e) == 1 ? 1 : 2;
    if (const char *e = get("HB_DOTQ_TILES")) k.dotq_tiles = std::max(1, atoi(e));
    if (const char *e = get("HB_DOTQ2_TILES")) { k.dotq2_tiles = std::max(1, atoi(e)); k.dotq2_tiles_set = true; }
    if (const char *e = get("HB_DOTQ2_KIND")) k.kind = std::max(0, std::min(2, atoi(e)));
    if (const char *e = get("HB_Q2M_CT")) k.q2m_ct = atoi(e) >= 16 ? 16 : atoi(e) >= 8 ? 8 : 4;
    if (const char *e = get("HB_Q2M_G")) k.q2m_g = atoi(e) == 3 ? 3 : atoi(e) >= 2 ? 2 : atoi(e) == 0 ? 0 : 1;
    if (const char *e = get("HB_Q2M_SC")) k.q2m_sc = atoi(e) != 0;
    if (const char *e = get("HB_DOTQ2_NC")) k.nc = std::max(4, atoi(e) / 4 * 4);
    if (const char *e = get("HB_DOTQ2_RS")) k.dotq2_rs = atoi(e) == 256 ? 256 : atoi(e) == 128 ? 128 : 512;
    return k;
}

// ---- the plan ----
struct hb_matvec_shape {
    int layout;       // 8: int8 columns (k_dotq), 2: 2-bit columns
    int64_t ld, ld2;  // bytes per column of X (a multiple of 256) and of X2
    int ncols;        // columns of this launch: whole panels
    int nupd, nfin;   // the update rows and finalize rows that ride in the launch
    bool dense;       // the update rows are the dense ones (update_rows_dense: HBU_LDS)
    int num_cus;
};

enum { HB_MV_DOTQ2 = 0, HB_MV_DOTQ2M = 1, HB_MV_DOTQ2R = 2, HB_MV_DOTQ = 3 };

struct hb_matvec_plan {
    int family;            // HB_MV_*
    int arg[3];            // its template arguments, in the order of its HB_*_KERNELS list (unused ones 0)
    int nstages, NS, ncg;  // stages of a column, stages per tile (k_dotq2r: columns per tile), column groups
    int tiles, blocks;     // tiles = ncg x rows of NS stages; blocks = update + finalize + tiles
    int lds;               // dynamic LDS bytes per block
};

static inline hb_matvec_plan plan_matvec(const hb_matvec_shape &s, const hb_matvec_knobs &k)
{
    hb_matvec_plan p{};
    const int ncols = s.ncols;
    auto tiled = [&](int family, int nst, int NS, int ncg, int tiles, int lds) {
        p.family = family, p.nstages = nst, p.NS = NS, p.ncg = ncg, p.tiles = tiles, p.blocks = s.nupd + s.nfin + tiles, p.lds = lds;
        return p;
    };
    if (s.layout != 2) {
        // tiles of one k_dotq launch: about three waves per compute unit, each a long run of stages (measured: fewer, longer
        // waves stream better than many short ones; tools/dotq_bench.hip)
        const int nst = (int)(s.ld / HBQ_RS), ncg = ncols / 64;
        const int ns = std::max(1, std::min(nst, (int)((double)k.dotq_tiles / ncg + 0.5)));
        // (int32 accumulators, digits in [-128, 127] against every int8 code, -128 included — hb_ctx_upload_genotype_i8 admits it:
        // NS * 128 rows * 128 * 128 < 2^31 holds up to NS = 1023; at 1024 a column of -128 on planes of -128 sums to 2^31 and wraps)
        const int NS = std::min(1023, (nst + ns - 1) / ns);
        return tiled(HB_MV_DOTQ, nst, NS, ncg, ncg * ((nst + NS - 1) / NS), s.dense ? HBU_LDS : HBQ_LDS);
    }
    // the 2-bit resident layout (hb_dotq2.hpp): about two long-lived waves per compute unit
    if (k.kind == 1) { // rows across the lanes, no LDS (k_dotq2r): tiles = row blocks x groups of NC columns
        int NC = k.nc;
        while (NC > Q2R_CB && ncols % NC) NC -= Q2R_CB; // (ends at Q2R_CB, which divides every panel width)
        const int ncg = ncols / NC, nst = (int)((s.ld2 * 4 + Q2R_RB - 1) / Q2R_RB);
        return tiled(HB_MV_DOTQ2R, nst, NC, ncg, ncg * nst, 0);
    }
    const bool mfma = k.kind == 2; // (A/B: the digit-plane product on the matrix cores, k_dotq2m; 256-individual stages, 64 columns per wave)
    int cpl = (ncols % 128 == 0 && !mfma && k.dotq2_rs != 128) ? k.dotq2_cpl : 1;
    // the matrix-core kernel's shape (hb_dotq2.hpp): column tiles of 16 per wave, stages requested together, one accumulator set per scale or one
    int q2m_ct = k.q2m_ct, q2m_g = k.q2m_g;
    while (mfma && q2m_ct > 4 && ncols % (16 * q2m_ct)) q2m_ct /= 2;
    if (q2m_ct == 16 && q2m_g == 2) q2m_g = 1;
    if ((q2m_g == 0 || q2m_g == 3) && (s.ld % 512 != 0 || ncols % 64)) q2m_g = 1; // (the 512-individual stages read whole stages of digits: the padded length must be a multiple)
    if (q2m_g == 0 || q2m_g == 3) q2m_ct = 4;
    const int RS = mfma ? ((q2m_g == 0 || q2m_g == 3) ? 512 : Q2M_RS) : k.dotq2_rs;
    const int nst = (int)((s.ld + RS - 1) / RS);
    const int ncg = mfma ? ncols / (16 * q2m_ct) : ncols / (64 * cpl);
    // (a tile is at least four stages: its first stage's load latency and its closing atomics are paid per tile)
    // (the matrix-core kernel streams best with few, long tiles — its per-stage work is an eighth of the v_dot4 kernel's, so a tile's fixed
    // costs weigh more: ~800 tiles per 3584-column launch)
    int ns = std::max(1, std::min(std::max(1, nst / 4), (int)((double)(mfma && !k.dotq2_tiles_set ? ((q2m_g == 0 || q2m_g == 3) ? 900 : 800) : k.dotq2_tiles) / ncg + 0.5)));
    // (int32 accumulators of genotypes scaled by up to 32 — Q2_SCALED, k_dotq2m. The scale-32 accumulator sees one row in four, 174 762 of
    // them at 96 x 128 stay below 2^31: the true bound of a tile is 4 x 2^31 / (96 x 128) = 699 050 individuals. The floor below keeps a
    // tile at 131 072, well inside it)
    ns = std::max(ns, (int)(((int64_t)nst * RS + 131071) / 131072));
    const int lds = mfma ? q2m_lds(q2m_ct, q2m_g) : q2_lds(cpl, RS);
    if (mfma && (q2m_g == 0 || q2m_g == 3) && !k.dotq2_tiles_set) {
        // ALL blocks of the launch resident at once (round 5, the last measurement of the round). A block of this kernel holds 37 KB of LDS: four per
        // compute unit, 128 per XCD — less the chain workgroup's compute unit and k_fwd's share of another, which sit on ONE XCD — and the
        // dispatcher deals the blocks round-robin over the eight XCDs whatever they have free. 784 tiles + 196 update + 56 finalize blocks = 1 036
        // is 130 per XCD: the XCD with the chain started its last nine tiles when its first ones ended, 8.4 us into a 9-us launch, and the launch
        // took 14.6 us in situ (tools/launch_roles.py). Fewer, longer tiles until the fullest XCD's share fits its slots: 12.6 us, 433 -> 454 sweeps/s.
        const int per_cu = std::max(1, std::min(8, (160 * 1024) / std::max(1, lds)));
        const int cus_per_xcd = std::max(1, s.num_cus / 8);
        const int budget = 8 * (cus_per_xcd * per_cu - (per_cu + 3)); // (the fullest XCD gets ceil(blocks / 8))
        auto total = [&](int kk) { const int NSk = (nst + kk - 1) / kk; return s.nupd + s.nfin + ncg * ((nst + NSk - 1) / NSk); };
        const int ns_min = std::max(1, (int)(((int64_t)nst * RS + 131071) / 131072));
        while (ns > ns_min && total(ns) > budget) ns--;
    }
    const int NS = (nst + ns - 1) / ns;
    p.arg[0] = mfma ? q2m_ct : cpl, p.arg[1] = mfma ? q2m_g : RS, p.arg[2] = mfma && k.q2m_sc;
    return tiled(mfma ? HB_MV_DOTQ2M : HB_MV_DOTQ2, nst, NS, ncg, ncg * ((nst + NS - 1) / NS), lds);
}
