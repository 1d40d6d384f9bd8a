// CMBlikes device structs and constants: what the host builds (cmblikes.hip) and the
// kernels of cmblfg.h, cmblwindow.h, cmblreduce.h, cmblhl.h and cmblexact.h read.
// (included by cmblikes.hip inside namespace cmamd)
#pragma once

static constexpr int CL_MAXMAPS = 16;          // HL matrices up to 16 x 16 in one wave
static constexpr int CL_MAXREQ = 32;            // required maps
static constexpr int BK_NPARAM = 16;            // BKPlanck.paramnames
static constexpr int WK_COLS = 32;              // window columns per work item (two 16-row MFMA blocks)
static constexpr int WK_CHUNK = 64;             // l per chunk
static constexpr int WK_NCH = 4;     // chunks per work item
static constexpr int WK_TS = WK_CHUNK + 2;      // LDS row stride of the spectrum tile (doubles)

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct CLPair {      // one required map pair (i >= j)
    int field;       // theory field index 0..9 (TT TE EE BT BE BB PT PE PB PP)
    int cmb;         // both theory indices <= B: aberration and calibration apply
    int fg;          // foregrounds: 0 none, 1 BK EE, 2 BK BB, 3 SMICA TT
    int mi, mj;      // required-map indices (0-based)
};

struct WItem {       // one (map pair, <= WK_NCH l chunks, <= WK_COLS window columns) contraction
    int pair;
    int l0, l1;      // l range (inclusive), l0 even when possible
    int ncol;
    int part;        // partial rows part .. part+ncol-1
    int nch;         // chunks of WK_CHUNK l
    long long woff;  // dense weights [nch][WK_CHUNK][WK_COLS] (zero padded)
    long long woff2; // direct-kernel weights [nch][ncol blocks][16 columns][WK_CHUNK] (zero padded)
};

struct BKMap {       // per required map: bandpass samples and constants (Read_Bandpass :72-105)
    int off, n;      // samples in bp_nu / bp_R / bp_dnu
    int bc;          // band-centre error slot: 0 none, 1 '95', 2 '150', 3 '220'
    int pad;
    double th_dust, th_sync, nu_bar;
};

struct CLDev {
    int lmin, lmax;                 // pcl_lmin, pcl_lmax
    int nitem;
    const WItem *items;
    const double *wdense;
    const double *wdirect;
    const CLPair *pairs;
    double aberration;
    int cal_index;                  // 0-based in DataParams, -1 none
    double log_cal_prior;           // > 0: add (ln cal / prior)^2 to chi^2
    // reduction to binned spectra, per element e = bin * ncl + cl
    int nE, ncl_used, nX, Np, approx, has_corr;
    const int *e_main_off, *e_main_rows, *e_corr_off, *e_corr_rows;   // partial rows per element
    const double *e_main_const, *e_corr_const;   // fixed-spectrum (fix_cl) window dots per element
    const double *fidcorr;          // [nE]
    const double *noise;            // [nE] (HL)
    const double *chat;             // [nE] (gaussian)
    const int *e_to_x;              // [nE] gaussian: index into bigX or -1
    // BK foregrounds
    int bk, nreq;
    int LP;                         // profile row length: prof[w][3][LP], indexed by l (zero outside lmin..lmax)
                                    // (SMICA: prof[w][0] = A1 exp(..), prof[w][1] = A2 (l/pivot)^n2)
    double smica_pivot;             // TSmica_planck%pivot (CMBlikes.f90:1270)
    const BKMap *bkmaps;
    const double *bp_nu, *bp_R, *bp_dnu;
    const double *bp_lnu;           // log(nu) of every bandpass sample
    int nsamp;                      // bandpass samples, all maps
    double *td_den;                 // [nsamp] exp(G nu / Td0) - 1 for the launch's first walker's Td0 (cmbl_bk_tdtab);
    double *td0;                    // [1] that Td0.  Both live in the call's workspace, so launches on other
                                    // streams with their own workspaces never share the table
    const double *log_l80;          // log(l / 80), l = 0 .. LP-1
    double fpivot_dust, fpivot_sync, decorr_dust[2], decorr_sync[2];
    int lform_dust, lform_sync;     // 0 flat, 1 lin, 2 quad
    // sparse evaluation (the sampler's per-likelihood change mask): walkers
    // [0, *wcount) of the launch are live, the rest exit; null = all W
    const int *wcount;
};

// live walkers of a launch over W (wcount: device count, or null)
__device__ __forceinline__ int live_walkers(const int *wcount, int W) { return wcount ? min(W, *wcount) : W; }

static constexpr double BK_TCMB = 2.72548;
static constexpr double BK_H = 6.62606957e-34;
static constexpr double BK_KB = 1.3806488e-23;
__host__ __device__ inline double ghz_kelvin() { return BK_H / BK_KB * 1e9; }

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// l per grouped item: 224 (BK15's l range in three items a pair group),
// cmbl_window_group 85.8 -> 78.1 us and configs[4] 396.4-397.8 -> 388.2-390.3
// us/step, against 160 / 192 / 256 / 320 / 608 (406 / 417-418 / 397 / 412-414 /
// 441 us/step; DESIGN.md section 5's table); 6 pairs per item 400-401
static constexpr int GP = 8;       // pairs per grouped item
static constexpr int GSEG = 224;   // l per grouped item (a multiple of 32)
static_assert(GSEG % 32 == 0, "grouped items are whole 32-l steps");
static_assert((GP * 16 * 16 / 2) % 256 == 0, "the weight staging moves GP * 16 rows of 16 l in whole passes");

struct GItem {
    int field, npair, l0, nstep;
    int pair[GP];       // CLPair index
    int ncol[GP];       // columns of each pair (<= 16)
    int part[GP];       // first partial row of each pair
    long long woff;     // weights [GP][16][nstep * 32] (zero padded)
};

// cmbl_gauss_small_kernel (cmblreduce.h): the partial rows of every element in tasks of <= 8 rows
struct SmallTask { int first, count; };      // rows e_*_rows[first .. first+count) (host side)
struct SmallDev {
    int ntask;
    const int *trow;                         // [ntask][8]: each task's partial rows, -1 padded
    const int *e_main_t, *e_corr_t;          // [nE+1] task ranges per element
};

struct HLDev {
    int n, m, nb, ncl, ncl_used, nX, Np;
    const double *chat;     // [nb][n][n]
    const double *cfhalf;   // [nb][n][n]
    const double *u0;       // [nb][n][n] eigenvectors (columns) of C_fid: the first eigensolve's starting basis
    const double *v0;       // [nb][n][n] eigenvectors of C_fid^-1/2 Chat C_fid^-1/2: the second's
    const int *cl_use;
    int *status;            // sticky CMBL_STATUS_* bits (cmbl_status)
    const int *wcount;      // live walkers (CLDev::wcount)
};

struct ExactDev {
    int n, ncl, lmin, lmax, bmin, nb, K;   // K: doubles per l row of tab
    int field[10], cmb[10];                // per element of the lower triangle (ElementsToMatrix order)
    const double *tab;                     // [nb][K]: N_l (ncl), R (ncl, lower packed), ln det Chat, (2l+1) fksy
    double aberration, log_cal_prior;
    int cal_index;
};
static constexpr int EXACT_MAXMAPS = 4;    // T, E, B, P
static constexpr int EXACT_WPB = 4;        // walkers per 256-thread block: one wave each
