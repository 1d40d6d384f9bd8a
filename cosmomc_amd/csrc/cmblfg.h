// CMBlikes foregrounds: the BK (TBK_planck) and SMICA (TSmica_planck) per-walker prologues.
// (included by cmblikes.hip inside namespace cmamd)
#pragma once

// Decorrelation (CMB_BK_Planck.f90:187-227)
__device__ inline double bk_decorr(double Delta, double nu0, double nu1, const double *piv, int l, int lform) {
    const double lpivot = 80.0;
    const double a = log(nu0 / nu1), b = log(piv[0] / piv[1]);
    const double scl_nu = (a * a) / (b * b);
    double scl_ell = 1.0;
    if (lform == 1) scl_ell = l / lpivot;
    else if (lform == 2) {
        const double t = l / lpivot;
        scl_ell = t * t;
    }
    if (Delta > 1.0) return 2.0 - exp(log(2.0 - Delta) * scl_nu * scl_ell);
    return exp(log(Delta) * scl_nu * scl_ell);
}

// The dust greybody's denominators exp(G nu / T_dust) - 1 of every bandpass
// sample at the first walker's T_dust (a fixed parameter in the BK15 runs, so
// every walker's): cmbl_bk_prologue takes them from here when its walker's
// T_dust is the same value -- the same operations, so the same bits -- and
// forms them itself otherwise.  One of its three exponentials per sample.
__global__ __launch_bounds__(256) void cmbl_bk_tdtab(CLDev c, const double *__restrict__ nuis)
{
    const double Tdust = nuis[4];   // DataParams(5) of walker 0 (row 0 exists whenever a prologue runs)
    const double G = ghz_kelvin();
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < c.nsamp) c.td_den[k] = exp(G * c.bp_nu[k] / Tdust) - 1;
    if (k == 0) c.td0[0] = Tdust;
}

// BK per-walker foreground set-up (TBK_planck_AddForegrounds :250-285): the
// SED factors of every map (one wave per map, bandpass integrals as wave
// reductions) and the dust / sync / dust-sync l profiles.
//   coef[w][3][nreq] = fdust, fsync, band-centre error;  prof[w][3][L]
static constexpr int BKP_THREADS = 256;   // a wave per map at a time
__global__ __launch_bounds__(BKP_THREADS) void cmbl_bk_prologue(CLDev c, const double *__restrict__ nuis, long long ld_nuis,
                                                       double *__restrict__ coef, double *__restrict__ prof, int W)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = blockIdx.x;
    if (w >= live_walkers(c.wcount, W)) return;
    const double *P = nuis + (long long)w * ld_nuis;
    const double Adust = P[0], Async = P[1], alphadust = P[2], betadust = P[3], Tdust = P[4];
    const double alphasync = P[5], betasync = P[6], dustsync_corr = P[7];
    const double G = ghz_kelvin();
    double *cw = coef + (long long)w * 3 * c.nreq;
    // pivot-frequency SEDs: the same for every map of this walker, so computed once
    const double nu0d = c.fpivot_dust, nu0s = c.fpivot_sync;
    const double gb0 = pow(nu0d, 3 + betadust) / (exp(G * nu0d / Tdust) - 1);
    const double pl0 = pow(nu0s, 2 + betasync);
    const bool tab = Tdust == c.td0[0];              // cmbl_bk_tdtab's denominators apply
    for (int i = wave; i < c.nreq; i += BKP_THREADS / 64) {
        const BKMap m = c.bkmaps[i];
        double gb = 0.0, pl = 0.0;
        for (int k = lane; k < m.n; k += 64) {
            const double nu = c.bp_nu[m.off + k], R = c.bp_R[m.off + k], dn = c.bp_dnu[m.off + k];
            const double lnu = c.bp_lnu[m.off + k];          // nu^e as exp(e log nu): one exp instead of a pow
            const double den = tab ? c.td_den[m.off + k] : exp(G * nu / Tdust) - 1;
            gb += dn * R * exp((3 + betadust) * lnu) / den;
            pl += dn * R * exp((2 + betasync) * lnu);
        }
        gb = wave_sum(gb);
        pl = wave_sum(pl);
        if (lane == 0) {
            double bc = 1.0;
            if (m.bc == 1) bc = P[12] + P[13] + 1.;
            else if (m.bc == 2) bc = P[12] + P[14] + 1.;
            else if (m.bc == 3) bc = P[12] + P[15] + 1.;
            double th_err = 1.0, gb_err = 1.0, pl_err = 1.0;
            if (bc != 1.) {                                   // DustScaling :130-141, SyncScaling :169-178
                const double e1 = exp(G * m.nu_bar / BK_TCMB) - 1, e2 = exp(G * m.nu_bar * bc / BK_TCMB) - 1;
                th_err = (bc * bc * bc * bc) * exp(G * m.nu_bar * (bc - 1) / BK_TCMB) * (e1 * e1) / (e2 * e2);
                gb_err = pow(bc, 3 + betadust) * (exp(G * m.nu_bar / Tdust) - 1) / (exp(G * m.nu_bar * bc / Tdust) - 1);
                pl_err = pow(bc, 2 + betasync);
            }
            cw[i] = (gb / gb0) / m.th_dust * (gb_err / th_err);
            cw[c.nreq + i] = (pl / pl0) / m.th_sync * (pl_err / th_err);
            cw[2 * c.nreq + i] = bc;
        }
    }
    const int LP = c.LP;
    double *pw = prof + (long long)w * 3 * LP;
    for (int l = tid; l < LP; l += blockDim.x) {
        if (l < c.lmin || l > c.lmax) {
            pw[l] = pw[LP + l] = pw[2 * LP + l] = 0.0;
            continue;
        }
        const double ll = c.log_l80[l];                     // (l/80)^a as exp(a log(l/80))
        pw[l] = Adust * exp(alphadust * ll);
        pw[LP + l] = Async * exp(alphasync * ll);
        pw[2 * LP + l] = dustsync_corr * sqrt(Adust * Async) * exp(((alphadust + alphasync) / 2) * ll);
    }
}

// SMICA's TT foreground (TSmica_planck_AddForegrounds, CMBlikes.f90:1295-1322)
// per walker and l as two profile rows, added to every TT map pair in window
// staging in the reference's order: (D_l + A1 exp(n1 lnr + n1run/2 lnr^2)) +
// A2 (l/pivot)^n2, lnr = ln(l/pivot).  prof[w][3][LP]; row 2 unused.
__global__ __launch_bounds__(256) void cmbl_smica_prologue(CLDev c, const double *__restrict__ nuis, long long ld_nuis,
                                                          double *__restrict__ prof, int W)
{
    const int w = blockIdx.y;
    if (w >= live_walkers(c.wcount, W)) return;
    const int l = blockIdx.x * 256 + threadIdx.x;
    const int LP = c.LP;
    if (l >= LP) return;
    const double *P = nuis + (long long)w * ld_nuis;
    double *pw = prof + (long long)w * 3 * LP;
    if (l < c.lmin || l > c.lmax) {
        pw[l] = pw[LP + l] = 0.0;
        return;
    }
    const double A1 = P[0], n1 = P[1], n1run = P[2], A2 = P[3], n2 = P[4];
    const double x = (double)l / c.smica_pivot;
    const double lnrat = log(x);
    pw[l] = A1 * exp(n1 * lnrat + n1run / 2 * (lnrat * lnrat));
    pw[LP + l] = A2 * pow(x, n2);
}

// TSmica_planck_derivedParameters (CMBlikes.f90:1324-1337): derived(1) =
// Cls(1,1)%CL(2000) of map cross-spectra initialised to zero plus the
// foregrounds, i.e. the TT foreground at l = 2000 when the first required map
// pair is TT (0 otherwise); any further derived columns 0 (the base
// TDataLikelihood_derivedParameters, GeneralTypes.f90:504-512).  NaN when
// l = 2000 is outside pcl_lmin..pcl_lmax (the reference reads out of bounds).
__global__ __launch_bounds__(64) void cmbl_smica_derived(CLDev c, int tt11, const double *__restrict__ nuis,
                                                        long long ld_nuis, double *__restrict__ out, long long ld_out,
                                                        int nd, int W)
{
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= W) return;
    const double *P = nuis + (long long)w * ld_nuis;
    double *o = out + (long long)w * ld_out;
    const int l = 2000;
    double v = 0.0;
    if (l < c.lmin || l > c.lmax) v = __builtin_nan("");
    else if (tt11) {
        const double A1 = P[0], n1 = P[1], n1run = P[2], A2 = P[3], n2 = P[4];
        const double x = (double)l / c.smica_pivot;
        const double lnrat = log(x);
        v = (v + A1 * exp(n1 * lnrat + n1run / 2 * (lnrat * lnrat))) + A2 * pow(x, n2);
    }
    o[0] = v;
    for (int k = 1; k < nd; k++) o[k] = 0.0;
}
