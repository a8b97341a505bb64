/* lsx_oracle.c -- TEST INFRASTRUCTURE, NOT THE PRODUCT.
 *
 * Scalar C restatement of Lightspinner's MALI hot path behind the lsx C ABI
 * (include/lsx.h).  It exists to (1) check the HIP kernels, (2) be the timed CPU
 * baseline in bench.py.  Only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg may load it; lightspinner_amd/ never does.
 *
 * Parity is PINNED: tests/test_oracle_golden.py checks this file against golden
 * vectors produced by importing the unmodified reference (tests/golden/make_golden.py).
 *
 * Every function cites the reference lines it restates; the floating-point
 * operation ORDER of the reference's numpy expressions is kept (build with
 * -ffp-contract=off) so results agree to a few ulp.
 *
 * Reference: /root/reference/formal_solver.py, rh_method.py, utils.py, constants.py
 */
#include "../include/lsx.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

/* constants.py:1-27 (values reproduced bit for bit) */
static const double CLight = 2.99792458E+08;
static const double HPlanck = 6.6260755E-34;
static const double KBoltzmann = 1.380658E-23;
static const double NM_TO_M = 1.0E-09;
#define HC (HPlanck * CLight)

static __thread char g_err[512];
static int fail(int code, const char* msg)
{
    snprintf(g_err, sizeof g_err, "%s", msg);
    return code;
}
const char* lsx_last_error(void) { return g_err; }
const char* lsx_backend_name(void) { return "oracle-c"; }
int32_t lsx_abi_version(void) { return LSX_ABI_VERSION; }
const char* lsx_build_id(void) { return "oracle-c"; }

struct lsx_ctx {
    int Nspace, Nrays, Nspect, Natoms, Ntrans, ncol;
    int NLtot, NL2tot, Nlines, SNl, SNc;
    int sca_per_lambda, phi_compact;
    int* Nlevel;
    int* lev_off;  /* [Natoms] offset into NLtot   */
    int* lev2_off; /* [Natoms] offset into NL2tot  */
    double *wavelength, *muz, *wmu;
    lsx_transition* trans;
    uint8_t* active;
    double* alpha;
    int* alpha_off; /* [Ntrans] offset into alpha (continua)          */
    int* phi_off;   /* [Ntrans] offset (in lambda points) into SNl    */
    int* line_idx;  /* [Ntrans] index among lines                      */
    /* per column, reference layouts */
    double *height, *temperature, *nStar, *nTotal, *n, *C, *bg_chi, *bg_eta, *bg_sca, *phi, *wphi;
    double *J, *I, *Gamma, *Rij, *Rji, *dJcol, *dPcol;
    double* spec_save;        /* what a speculative formal solution overwrote (lsx_formal_sol_gamma_speculative), or NULL */
    double spec_last_dJ;
    int spec_valid;
    double mon_dJ, mon_dP;    /* the maxima as they were at lsx_sync_begin */
    int mon_set, mon_spec;
    double* mon_n;            /* the populations as they were at lsx_sync_begin_populations, or NULL */
    int mon_n_pending, mon_n_valid;
    long* sing_col; /* per column: (depth << 8 | atom) of its first singular system in the last stat_equil, or -1 */
    /* set-up chain: deep copy of the atomic data (lsx_set_atomic_data) and what lsx_set_atmosphere derives */
    int have_atomic_data;
    int solver;                  /* LSX_SOLVER_* (N4) */
    double weight_H, weight_He, abundance_He;
    lsx_atom_model* am;       /* [Natoms]; levels / lines / collisions (with their tables) owned */
    double *vBroad, *aDamp;   /* [col][Natoms][k], [col][Nlines][k] */
    int nthreads;
    uint8_t* colmask; /* NULL = all active */
    double last_dJ, last_dP;
};

static void free_atomic_data(lsx_ctx* c);

static size_t phi_per_col(const lsx_ctx* c)
{
    return (size_t)c->SNl * (c->phi_compact ? 1 : (size_t)c->Nrays * 2) * c->Nspace;
}
static size_t sca_per_col(const lsx_ctx* c)
{
    return (size_t)(c->sca_per_lambda ? c->Nspect : 1) * c->Nspace;
}

int lsx_create(const lsx_problem* d, int32_t ncol, int32_t device, void* stream, lsx_ctx** out)
{
    (void)device;
    (void)stream;
    if (!d || !out || ncol < 1) return fail(LSX_EINVAL, "lsx_create: null argument or ncol < 1");
    if (d->abi_version != LSX_ABI_VERSION) return fail(LSX_EINVAL, "lsx_create: ABI version mismatch");
    if (d->Nspace < 3) return fail(LSX_EINVAL, "lsx_create: Nspace must be >= 3 (formal_solver.py:120-139)");
    if (d->Nrays < 1 || d->Nspect < 1 || d->Natoms < 1 || d->Ntrans < 0)
        return fail(LSX_EINVAL, "lsx_create: bad dimensions");
    lsx_ctx* c = (lsx_ctx*)calloc(1, sizeof *c);
    c->Nspace = d->Nspace; c->Nrays = d->Nrays; c->Nspect = d->Nspect;
    c->Natoms = d->Natoms; c->Ntrans = d->Ntrans; c->ncol = ncol;
    c->sca_per_lambda = d->sca_per_lambda; c->phi_compact = d->phi_compact;
    c->Nlevel = (int*)malloc(sizeof(int) * c->Natoms);
    c->lev_off = (int*)malloc(sizeof(int) * c->Natoms);
    c->lev2_off = (int*)malloc(sizeof(int) * c->Natoms);
    for (int a = 0; a < c->Natoms; ++a) {
        c->Nlevel[a] = d->Nlevel[a];
        c->lev_off[a] = c->NLtot; c->lev2_off[a] = c->NL2tot;
        c->NLtot += d->Nlevel[a]; c->NL2tot += d->Nlevel[a] * d->Nlevel[a];
    }
#define DUP(dst, src, cnt, T) do { dst = (T*)malloc(sizeof(T) * (size_t)(cnt)); memcpy(dst, src, sizeof(T) * (size_t)(cnt)); } while (0)
    DUP(c->wavelength, d->wavelength, c->Nspect, double);
    DUP(c->muz, d->muz, c->Nrays, double);
    DUP(c->wmu, d->wmu, c->Nrays, double);
    DUP(c->trans, d->trans, c->Ntrans > 0 ? c->Ntrans : 1, lsx_transition);
    DUP(c->active, d->active, (size_t)(c->Ntrans > 0 ? c->Ntrans : 1) * c->Nspect, uint8_t);
    c->alpha_off = (int*)calloc(c->Ntrans + 1, sizeof(int));
    c->phi_off = (int*)calloc(c->Ntrans + 1, sizeof(int));
    c->line_idx = (int*)calloc(c->Ntrans + 1, sizeof(int));
    for (int t = 0; t < c->Ntrans; ++t) {
        const lsx_transition* tr = &c->trans[t];
        if (tr->atom < 0 || tr->atom >= c->Natoms || tr->i < 0 || tr->j >= c->Nlevel[tr->atom] || tr->i >= tr->j ||
            tr->Nblue < 0 || tr->Nlambda < 2 || tr->Nblue + tr->Nlambda > c->Nspect) {
            lsx_destroy(c);
            return fail(LSX_EINVAL, "lsx_create: inconsistent transition table entry");
        }
        if (tr->is_line) { c->phi_off[t] = c->SNl; c->line_idx[t] = c->Nlines; c->SNl += tr->Nlambda; c->Nlines++; }
        else { c->alpha_off[t] = c->SNc; c->SNc += tr->Nlambda; }
    }
    DUP(c->alpha, d->alpha, c->SNc > 0 ? c->SNc : 1, double);
#undef DUP
    size_t nc = (size_t)ncol, Ns = (size_t)c->Nspace;
    c->height = (double*)calloc(nc * Ns, 8); c->temperature = (double*)calloc(nc * Ns, 8);
    c->nStar = (double*)calloc(nc * c->NLtot * Ns, 8); c->n = (double*)calloc(nc * c->NLtot * Ns, 8);
    c->nTotal = (double*)calloc(nc * c->Natoms * Ns, 8);
    c->C = (double*)calloc(nc * c->NL2tot * Ns, 8); c->Gamma = (double*)calloc(nc * c->NL2tot * Ns, 8);
    c->bg_chi = (double*)calloc(nc * c->Nspect * Ns, 8); c->bg_eta = (double*)calloc(nc * c->Nspect * Ns, 8);
    c->bg_sca = (double*)calloc(nc * sca_per_col(c), 8);
    c->phi = (double*)calloc(nc * (phi_per_col(c) ? phi_per_col(c) : 1), 8);
    c->wphi = (double*)calloc(nc * (c->Nlines ? c->Nlines : 1) * Ns, 8);
    c->J = (double*)calloc(nc * c->Nspect * Ns, 8); c->I = (double*)calloc(nc * c->Nspect * c->Nrays, 8);
    c->Rij = (double*)calloc(nc * (c->Ntrans ? c->Ntrans : 1) * Ns, 8);
    c->Rji = (double*)calloc(nc * (c->Ntrans ? c->Ntrans : 1) * Ns, 8);
    c->dJcol = (double*)calloc(nc, 8); c->dPcol = (double*)calloc(nc, 8);
    c->sing_col = (long*)calloc(nc, sizeof(long));
    for (size_t q = 0; q < nc; ++q) c->sing_col[q] = -1;
    c->nthreads = 1;
    *out = c;
    return LSX_OK;
}

void lsx_destroy(lsx_ctx* c)
{
    if (!c) return;
    free(c->Nlevel); free(c->lev_off); free(c->lev2_off); free(c->wavelength); free(c->muz); free(c->wmu);
    free(c->trans); free(c->active); free(c->alpha); free(c->alpha_off); free(c->phi_off); free(c->line_idx);
    free(c->height); free(c->temperature); free(c->nStar); free(c->nTotal); free(c->n); free(c->C);
    free(c->bg_chi); free(c->bg_eta); free(c->bg_sca); free(c->phi); free(c->wphi);
    free(c->colmask);
    free(c->J); free(c->I); free(c->Gamma); free(c->Rij); free(c->Rji); free(c->dJcol); free(c->dPcol); free(c->sing_col);
    free_atomic_data(c); free(c->vBroad); free(c->aDamp); free(c->spec_save); free(c->mon_n);
    free(c);
}

/* oracle-only knob: number of OpenMP threads used over columns (default 1) */
int lsx_oracle_set_threads(lsx_ctx* c, int32_t n)
{
    if (!c || n < 1) return fail(LSX_EINVAL, "lsx_oracle_set_threads: bad argument");
    c->nthreads = n;
    return LSX_OK;
}

int lsx_set_columns(lsx_ctx* c, int32_t col0, int32_t ncol, const lsx_columns* s)
{
    if (!c || !s || col0 < 0 || ncol < 1 || col0 + ncol > c->ncol) return fail(LSX_EINVAL, "lsx_set_columns: bad range");
    size_t Ns = c->Nspace, o = (size_t)col0, n = (size_t)ncol;
#define CP(dst, src, per) do { if (!(src)) return fail(LSX_EINVAL, "lsx_set_columns: null " #src); memcpy(dst + o * (per), src, n * (per) * 8); } while (0)
    CP(c->height, s->height, Ns); CP(c->temperature, s->temperature, Ns);
    CP(c->nStar, s->nStar, c->NLtot * Ns); CP(c->nTotal, s->nTotal, c->Natoms * Ns); CP(c->n, s->n, c->NLtot * Ns);
    CP(c->C, s->C, c->NL2tot * Ns); CP(c->bg_chi, s->bg_chi, c->Nspect * Ns); CP(c->bg_eta, s->bg_eta, c->Nspect * Ns);
    CP(c->bg_sca, s->bg_sca, sca_per_col(c));
    if (c->Nlines && (s->phi || s->wphi)) { CP(c->phi, s->phi, phi_per_col(c)); CP(c->wphi, s->wphi, c->Nlines * Ns); }
#undef CP
    memset(c->J + o * c->Nspect * Ns, 0, n * c->Nspect * Ns * 8);   /* rh_method.py:562 */
    memset(c->I + o * c->Nspect * c->Nrays, 0, n * c->Nspect * c->Nrays * 8);
    memset(c->Rij + o * c->Ntrans * Ns, 0, n * c->Ntrans * Ns * 8);  /* rh_method.py:130-131 */
    memset(c->Rji + o * c->Ntrans * Ns, 0, n * c->Ntrans * Ns * 8);
    return LSX_OK;
}

/* ---- Voigt function H(a, v) = Re w(v + i a), a > 0 (utils.py:13-15 calls scipy's wofz) ------
 * Trapezoid rule with step h on w(z) = (i/pi) int exp(-t^2)/(z - t) dt plus the residue of the
 * pole the contour crosses (Chiarella & Reichel 1968; Matta & Reichel 1971):
 *   H = (h a/pi) sum_n exp(-g_n^2) / ((v - g_n)^2 + a^2) + Re[ 2 exp(-z^2) / (1 -+ exp(-2 pi i z/h)) ]
 * on the grid g_n = n h (sign -) or (n + 1/2) h (sign +), whichever keeps v at least h/4 away from
 * a node; error ~ exp(-pi^2/h^2) = 7e-18 for h = 1/2.  All terms of the sum are positive. */
static double voigt_H(double a, double v)
{
    const double h = 0.5, pi = 3.14159265358979323846;
    double x = fabs(v);
    double t = x / h, fr = t - floor(t);
    int half = !(fr >= 0.25 && fr < 0.75);
    double shift = half ? 0.5 : 0.0;
    double s = 0.0;
    for (int n = -14; n <= 13; ++n) {
        double g = (n + shift) * h;
        double d = x - g;
        s += exp(-g * g) / (d * d + a * a);
    }
    double H = h * a / pi * s;
    if (x < 27.0 && a < pi / h) {
        /* exp(-z^2) = exp(a^2 - x^2) (cos 2xa - i sin 2xa);  exp(-2 pi i z/h) = exp(2 pi a/h) (cos - i sin)(2 pi x/h) */
        double er = exp(a * a - x * x), c1 = cos(2.0 * x * a), s1 = -sin(2.0 * x * a);
        double E = exp(2.0 * pi * a / h), th = 2.0 * pi * x / h;
        double sg = half ? 1.0 : -1.0;
        double dr = 1.0 + sg * E * cos(th), di = -sg * E * sin(th);
        /* Re[(c1 + i s1) / (dr + i di)] */
        H += 2.0 * er * (c1 * dr + s1 * di) / (dr * dr + di * di);
    }
    return H;
}

double lsx_oracle_voigt(double a, double v) { return voigt_H(a, v); }

/* Oracle-only: t.Rij / t.Rji of column `col` (rh_method.py:691-692), [Ntrans][Nspace] each.  Not part of the ABI (the
 * reference never reads them); the golden files hold them and they pin the oracle's intensity at EVERY depth. */
int lsx_oracle_rates(lsx_ctx* c, int32_t col, double* Rij, double* Rji)
{
    if (!c || col < 0 || col >= c->ncol || !Rij || !Rji) return fail(LSX_EINVAL, "lsx_oracle_rates: bad argument");
    size_t per = (size_t)c->Ntrans * c->Nspace;
    memcpy(Rij, c->Rij + per * col, per * 8);
    memcpy(Rji, c->Rji + per * col, per * 8);
    return LSX_OK;
}

/* rh_method.py:198-243 */
int lsx_set_line_profiles(lsx_ctx* c, int32_t col0, int32_t ncol, const double* aDamp, const double* vBroad,
                          const double* vlos)
{
    if (!c || !aDamp || !vBroad || col0 < 0 || ncol < 1 || col0 + ncol > c->ncol)
        return fail(LSX_EINVAL, "lsx_set_line_profiles: bad argument");
    if (c->phi_compact && vlos) return fail(LSX_EINVAL, "lsx_set_line_profiles: a phi_compact context takes vlos == NULL");
    const double CLight = 2.99792458E+08, sqrtPi = 1.7724538509055160273;
    const int Ns = c->Nspace, Nrays = c->Nrays;
    for (int cc = 0; cc < ncol; ++cc) {
        size_t col = (size_t)col0 + cc;
        double* phi = c->phi + col * phi_per_col(c);
        for (int kr = 0; kr < c->Ntrans; ++kr) {
            const lsx_transition* t = &c->trans[kr];
            if (!t->is_line) continue;
            const int li = c->line_idx[kr];
            const double* ad = aDamp + ((size_t)cc * c->Nlines + li) * Ns;
            const double* vb = vBroad + ((size_t)cc * c->Natoms + t->atom) * Ns;
            const double* wl = c->wavelength + t->Nblue;
            double* wphi = c->wphi + (col * c->Nlines + li) * Ns;
            for (int k = 0; k < Ns; ++k) wphi[k] = 0.0;
            for (int la = 0; la < t->Nlambda; ++la) {
                /* wlambda, rh_method.py:157-196 */
                double wla = (la == 0) ? 0.5 * (wl[1] - wl[0]) : (la == t->Nlambda - 1) ? 0.5 * (wl[la] - wl[la - 1]) : 0.5 * (wl[la + 1] - wl[la - 1]);
                wla *= CLight / t->lambda0;
                for (int mu = 0; mu < (c->phi_compact ? 1 : Nrays); ++mu)
                    for (int d = 0; d < (c->phi_compact ? 1 : 2); ++d) {
                        double* ph = c->phi_compact ? phi + ((size_t)c->phi_off[kr] + la) * Ns
                                                    : phi + ((((size_t)c->phi_off[kr] + la) * Nrays + mu) * 2 + d) * Ns;
                        for (int k = 0; k < Ns; ++k) {
                            double v = (wl[la] - t->lambda0) * CLight / (vb[k] * t->lambda0);
                            double vl = vlos ? vlos[(size_t)cc * Ns + k] : 0.0;
                            double vk = v + (d ? 1.0 : -1.0) * (c->muz[mu] * vl / vb[k]);
                            double p = voigt_H(ad[k], vk) / (sqrtPi * vb[k]);
                            ph[k] = p;
                            if (!c->phi_compact) wphi[k] += p * (wla * 0.5 * c->wmu[mu]);
                        }
                    }
                if (c->phi_compact) {   /* same value for every ray and direction: the weights sum over them */
                    const double* ph = phi + ((size_t)c->phi_off[kr] + la) * Ns;
                    for (int mu = 0; mu < Nrays; ++mu)
                        for (int d = 0; d < 2; ++d)
                            for (int k = 0; k < Ns; ++k) wphi[k] += ph[k] * (wla * 0.5 * c->wmu[mu]);
                }
            }
            for (int k = 0; k < Ns; ++k) wphi[k] = 1.0 / wphi[k];
        }
    }
    return LSX_OK;
}

/* ---- set-up chain -------------------------------------------------------------------------------- */
static const double Amu = 1.6605402E-27, MElectron = 9.1093897E-31, QElectron = 1.60217733E-19, Epsilon0 = 8.854187817E-12,
                    RBohr = 5.29177349E-11, ERydberg = 2.1798741E-18, ABarH = 7.42E-41, CM_TO_M = 1.0E-02;

static void free_atomic_data(lsx_ctx* c)
{
    if (!c->am) return;
    for (int a = 0; a < c->Natoms; ++a) {
        for (int q = 0; q < c->am[a].Ncollision; ++q) {
            free((void*)c->am[a].collisions[q].temperature);
            free((void*)c->am[a].collisions[q].rates);
        }
        free((void*)c->am[a].levels); free((void*)c->am[a].lines); free((void*)c->am[a].collisions);
    }
    free(c->am);
    c->am = NULL;
    c->have_atomic_data = 0;
}

static void* dup_bytes(const void* p, size_t n)
{
    void* q = malloc(n ? n : 1);
    if (n) memcpy(q, p, n);
    return q;
}

int lsx_set_atomic_data(lsx_ctx* c, const lsx_atomic_data* d)
{
    if (!c || !d || !d->atoms) return fail(LSX_EINVAL, "lsx_set_atomic_data: null argument");
    if (d->Natoms != c->Natoms) return fail(LSX_EINVAL, "lsx_set_atomic_data: number of atoms differs from the context's");
    for (int a = 0; a < c->Natoms; ++a) {
        const lsx_atom_model* m = &d->atoms[a];
        int nl = 0;
        for (int t = 0; t < c->Ntrans; ++t) nl += c->trans[t].is_line && c->trans[t].atom == a;
        if (m->Nlevel != c->Nlevel[a] || m->Nline != nl || !(m->weight > 0.0)) return fail(LSX_EINVAL, "lsx_set_atomic_data: atom does not match the context");
        for (int q = 0; q < m->Ncollision; ++q) {
            const lsx_collision* K = &m->collisions[q];
            if (K->nT < 2 || K->nT == 3 || K->i < 0 || K->j >= m->Nlevel || K->i >= K->j || !K->temperature || !K->rates)
                return fail(LSX_EINVAL, "lsx_set_atomic_data: inconsistent collision");
            /* the reference's interp1d sorts its table; a descending or repeated temperature is refused, as the HIP library does */
            for (int e = 1; e < K->nT; ++e)
                if (!(K->temperature[e] > K->temperature[e - 1])) return fail(LSX_EINVAL, "lsx_set_atomic_data: temperatures must ascend");
        }
    }
    free_atomic_data(c);
    if (c->Natoms < 1) return fail(LSX_EINVAL, "lsx_set_atomic_data: the context has no atoms");
    c->am = (lsx_atom_model*)calloc((size_t)c->Natoms, sizeof(lsx_atom_model));
    for (int a = 0; a < c->Natoms; ++a) {
        const lsx_atom_model* m = &d->atoms[a];
        c->am[a] = *m;
        c->am[a].levels = (const lsx_level*)dup_bytes(m->levels, sizeof(lsx_level) * (size_t)m->Nlevel);
        c->am[a].lines = (const lsx_line_model*)dup_bytes(m->lines, sizeof(lsx_line_model) * (size_t)m->Nline);
        lsx_collision* K = (lsx_collision*)dup_bytes(m->collisions, sizeof(lsx_collision) * (size_t)m->Ncollision);
        for (int q = 0; q < m->Ncollision; ++q) {
            K[q].temperature = (const double*)dup_bytes(m->collisions[q].temperature, 8 * (size_t)K[q].nT);
            K[q].rates = (const double*)dup_bytes(m->collisions[q].rates, 8 * (size_t)K[q].nT);
        }
        c->am[a].collisions = K;
    }
    c->weight_H = d->weight_H; c->weight_He = d->weight_He; c->abundance_He = d->abundance_He;
    c->have_atomic_data = 1;
    return LSX_OK;
}

/* VdwUnsold.setup, atomic_model.py:166-194 -> the temperature-independent cross-section */
static double unsold_cross(const lsx_ctx* c, const lsx_atom_model* m, const lsx_line_model* L)
{
    const lsx_level *up = &m->levels[L->j], *lo = &m->levels[L->i];
    int Z = up->stage + 1, ic = L->j + 1;
    while (m->levels[ic].stage < Z) ic += 1;
    const lsx_level* cont = &m->levels[ic];
    double deltaR = pow(ERydberg / (cont->E_SI - up->E_SI), 2.0) - pow(ERydberg / (cont->E_SI - lo->E_SI), 2.0);
    double fourPiEps0 = 4.0 * M_PI * Epsilon0;
    double C625 = pow(2.5 * QElectron * QElectron / fourPiEps0 * ABarH / fourPiEps0 * 2 * M_PI * pow(Z * RBohr, 2.0) / HPlanck * deltaR, 0.4);
    double vRel35He = pow(8.0 * KBoltzmann / (M_PI * Amu * m->weight) * (1.0 + m->weight / c->weight_He), 0.3);
    double vRel35H = pow(8.0 * KBoltzmann / (M_PI * Amu * m->weight) * (1.0 + m->weight / c->weight_H), 0.3);
    return 8.08 * (L->vdw[0] * vRel35H + L->vdw[1] * c->abundance_He * vRel35He) * C625;
}

/* VoigtLine.stark_broaden, atomic_model.py:318-345, at one depth */
static double stark_broaden(const lsx_atom_model* m, const lsx_line_model* L, double T, double ne)
{
    const lsx_level *up = &m->levels[L->j], *lo = &m->levels[L->i];
    double stark;
    if (L->stark > 0.0) {
        double weight = m->weight;
        double C = 8.0 * KBoltzmann / (M_PI * Amu * weight);
        double Cm = pow(1.0 + weight / (MElectron / Amu), 1.0 / 6.0);
        Cm += pow(1.0 + weight / 28.0, 1.0 / 6.0);
        int Z = lo->stage + 1, ic = L->i + 1;
        while (ic < m->Nlevel && m->levels[ic].stage < Z) ic += 1;
        double E_Ryd = ERydberg / (1.0 + MElectron / (weight * Amu));
        double neff_l = Z * sqrt(E_Ryd / (m->levels[ic].E_SI - lo->E_SI));
        double neff_u = Z * sqrt(E_Ryd / (m->levels[ic].E_SI - up->E_SI));
        double C4 = QElectron * QElectron / (4.0 * M_PI * Epsilon0) * RBohr * (2.0 * M_PI * RBohr * RBohr / HPlanck) / (18.0 * pow((double)Z, 4.0)) *
                    (pow(neff_u * (5.0 * neff_u * neff_u + 1.0), 2.0) - pow(neff_l * (5.0 * neff_l * neff_l + 1.0), 2.0));
        double cStark23 = 11.37 * pow(L->stark * C4, 2.0 / 3.0);
        double vRel = pow(C * T, 1.0 / 6.0) * Cm;
        stark = cStark23 * vRel * ne;
    } else if (L->stark < 0.0) {
        stark = fabs(L->stark) * ne;
    } else {
        stark = 0.0;
    }
    if (m->is_hydrogen) { /* linear_stark_broaden, :307-316 */
        int nUpper = (int)lround(sqrt(0.5 * up->g)), nLower = (int)lround(sqrt(0.5 * lo->g));
        double a1 = (nUpper - nLower == 1) ? 0.642 : 1.0;
        double Cl = a1 * 0.6 * (nUpper * nUpper - nLower * nLower) * CM_TO_M * CM_TO_M;
        stark += Cl * pow(ne, 2.0 / 3.0);
    }
    return stark;
}

/* the not-a-knot cubic scipy.interpolate.interp1d(x, y, kind=3) builds (make_interp_spline, k = 3), evaluated through its
 * second derivatives M; two points: linear.  fill_value = (y[0], y[-1]) outside the grid (collisional_rates.py:15-19) */
static void spline_moments(int n, const double* x, const double* y, double* M)
{
    for (int i = 0; i < n; ++i) M[i] = 0.0;
    if (n < 4) return;
    double* A = (double*)calloc((size_t)n * n + n, sizeof(double));   /* n x n system, then b: a table of any length */
    double* b = A + (size_t)n * n;
#define H(i) (x[(i) + 1] - x[(i)])
    A[0] = H(1); A[1] = -(H(0) + H(1)); A[2] = H(0); b[0] = 0.0;
    A[(n - 1) * n + n - 3] = H(n - 2); A[(n - 1) * n + n - 2] = -(H(n - 3) + H(n - 2)); A[(n - 1) * n + n - 1] = H(n - 3); b[n - 1] = 0.0;
    for (int i = 1; i < n - 1; ++i) {
        A[i * n + i - 1] = H(i - 1); A[i * n + i] = 2.0 * (H(i - 1) + H(i)); A[i * n + i + 1] = H(i);
        b[i] = 6.0 * ((y[i + 1] - y[i]) / H(i) - (y[i] - y[i - 1]) / H(i - 1));
    }
#undef H
    for (int col = 0; col < n; ++col) {
        int p = col;
        for (int r = col + 1; r < n; ++r) if (fabs(A[r * n + col]) > fabs(A[p * n + col])) p = r;
        if (p != col) { for (int q = 0; q < n; ++q) { double t = A[col * n + q]; A[col * n + q] = A[p * n + q]; A[p * n + q] = t; } double t = b[col]; b[col] = b[p]; b[p] = t; }
        for (int r = col + 1; r < n; ++r) {
            double f = A[r * n + col] / A[col * n + col];
            for (int q = col; q < n; ++q) A[r * n + q] -= f * A[col * n + q];
            b[r] -= f * b[col];
        }
    }
    for (int r = n - 1; r >= 0; --r) { double sacc = b[r]; for (int q = r + 1; q < n; ++q) sacc -= A[r * n + q] * M[q]; M[r] = sacc / A[r * n + r]; }
    free(A);
}
static double spline_eval(int n, const double* x, const double* y, const double* M, double t)
{
    if (t < x[0]) return y[0];
    if (t > x[n - 1]) return y[n - 1];
    int i = 0;
    while (i < n - 2 && t > x[i + 1]) ++i;
    double h = x[i + 1] - x[i], a = x[i + 1] - t, b = t - x[i];
    return (M[i] * a * a * a + M[i + 1] * b * b * b) / (6.0 * h) + (y[i] / h - M[i] * h / 6.0) * a + (y[i + 1] / h - M[i + 1] * h / 6.0) * b;
}

int lsx_set_atmosphere(lsx_ctx* c, int32_t col0, int32_t ncol, const lsx_atmosphere* s)
{
    if (!c || !s || col0 < 0 || ncol < 1 || col0 + ncol > c->ncol) return fail(LSX_EINVAL, "lsx_set_atmosphere: bad range");
    if (!c->have_atomic_data) return fail(LSX_EINVAL, "lsx_set_atmosphere: lsx_set_atomic_data has not been called");
    if (!s->temperature || !s->ne || !s->vturb || !s->nHGround || !s->nTotal) return fail(LSX_EINVAL, "lsx_set_atmosphere: null array pointer");
    if (c->phi_compact && s->vlos) return fail(LSX_EINVAL, "lsx_set_atmosphere: a phi_compact context takes vlos == NULL");
    const int Ns = c->Nspace;
    if (!c->vBroad) {
        c->vBroad = (double*)calloc((size_t)c->ncol * c->Natoms * Ns, 8);
        c->aDamp = (double*)calloc((size_t)c->ncol * (c->Nlines ? c->Nlines : 1) * Ns, 8);
    }
    for (int cc = 0; cc < ncol; ++cc) {
        const size_t col = (size_t)col0 + cc;
        const double *T = s->temperature + (size_t)cc * Ns, *ne = s->ne + (size_t)cc * Ns, *vt = s->vturb + (size_t)cc * Ns,
                     *nH = s->nHGround + (size_t)cc * Ns;
        memcpy(c->temperature + col * Ns, T, 8 * (size_t)Ns);
        memcpy(c->nTotal + col * c->Natoms * Ns, s->nTotal + (size_t)cc * c->Natoms * Ns, 8 * (size_t)c->Natoms * Ns);
        int line0 = 0;
        for (int a = 0; a < c->Natoms; ++a) {
            const lsx_atom_model* m = &c->am[a];
            double* vB = c->vBroad + (col * c->Natoms + a) * Ns;
            /* v_broad, atomic_model.py:66-69 */
            double vTherm = 2.0 * KBoltzmann / (Amu * m->weight);
            for (int k = 0; k < Ns; ++k) vB[k] = sqrt(vTherm * T[k] + vt[k] * vt[k]);
            /* damping, :491-502 */
            for (int q = 0; q < m->Nline; ++q) {
                const lsx_line_model* L = &m->lines[q];
                double cross = L->vdw_kind == 1 ? unsold_cross(c, m, L) : 0.0;
                double cDop = (HC / (m->levels[L->j].E_SI - m->levels[L->i].E_SI)) / (4.0 * M_PI);
                double* aD = c->aDamp + (col * c->Nlines + line0 + q) * Ns;
                for (int k = 0; k < Ns; ++k) {
                    double Qelast = 0.0;
                    if (L->vdw_kind == 1) Qelast += cross * pow(T[k], 0.3) * nH[k];            /* :197-198 */
                    Qelast += stark_broaden(m, L, T[k], ne[k]);
                    aD[k] = (L->gRad + Qelast) * cDop / vB[k];
                }
            }
            line0 += m->Nline;
            /* lte_pops, atomic_set.py:105-145 */
            double* nStar = c->nStar + (col * c->NLtot + c->lev_off[a]) * Ns;
            if (s->lte_pops) {
                double c1 = (HPlanck / (2.0 * M_PI * MElectron)) * (HPlanck / KBoltzmann);
                double c2 = sqrt(8.0 * M_PI / KBoltzmann) * pow(QElectron * QElectron / (4.0 * M_PI * Epsilon0), 1.5);
                double* nn = c->n + (col * c->NLtot + c->lev_off[a]) * Ns;
                const double* nTot = c->nTotal + (col * c->Natoms + a) * Ns;
                for (int k = 0; k < Ns; ++k) {
                    double dEion = c2 * sqrt(ne[k] / T[k]);
                    double cNe_T = 0.5 * ne[k] * pow(c1 / T[k], 1.5);
                    double total = 1.0;
                    for (int i = 1; i < m->Nlevel; ++i) {
                        double nDebye = 0.0;
                        int Z = m->levels[i].stage;
                        for (int mm = 1; mm < m->levels[i].stage - m->levels[0].stage + 1; ++mm) { nDebye += Z; Z += 1; }
                        double dE = m->levels[i].E_SI - m->levels[0].E_SI;
                        double gi0 = m->levels[i].g / m->levels[0].g;
                        int dZ = m->levels[i].stage - m->levels[0].stage;
                        double dE_kT = (dE - nDebye * dEion) / (KBoltzmann * T[k]);
                        double nst = gi0 * exp(-dE_kT);
                        nst /= (dZ == 0 ? 1.0 : dZ == 1 ? cNe_T : dZ == 2 ? cNe_T * cNe_T : pow(cNe_T, (double)dZ));
                        nStar[(size_t)i * Ns + k] = nst;
                        total += nst;
                    }
                    nStar[k] = nTot[k] / total;
                    for (int i = 1; i < m->Nlevel; ++i) nStar[(size_t)i * Ns + k] *= nStar[k];
                    for (int i = 0; i < m->Nlevel; ++i) nn[(size_t)i * Ns + k] = nStar[(size_t)i * Ns + k];
                }
            }
            /* compute_collisions, rh_method.py:474-487 */
            const int Nl = m->Nlevel;
            double* Cm = c->C + (col * c->NL2tot + c->lev2_off[a]) * Ns;
            for (size_t e = 0; e < (size_t)Nl * Nl * Ns; ++e) Cm[e] = 0.0;
            for (int q = 0; q < m->Ncollision; ++q) {
                const lsx_collision* K = &m->collisions[q];
                double* M = (double*)malloc(sizeof(double) * (size_t)K->nT);
                spline_moments(K->nT, K->temperature, K->rates, M);
                const lsx_level *jL = &m->levels[K->j], *iL = &m->levels[K->i];
                for (int k = 0; k < Ns; ++k) {
                    double Cv = spline_eval(K->nT, K->temperature, K->rates, M, T[k]);
                    double nsi = nStar[(size_t)K->i * Ns + k], nsj = nStar[(size_t)K->j * Ns + k];
                    double* Cij = &Cm[((size_t)K->i * Nl + K->j) * Ns + k];
                    double* Cji = &Cm[((size_t)K->j * Nl + K->i) * Ns + k];
                    if (K->kind == LSX_COLL_OMEGA) {                                       /* collisional_rates.py:38-45 */
                        double C0 = ERydberg / sqrt(MElectron) * M_PI * RBohr * RBohr * sqrt(8.0 / (M_PI * KBoltzmann));
                        double Cdown = C0 * ne[k] * Cv / (jL->g * sqrt(T[k]));
                        *Cij += Cdown;
                        *Cji += Cdown * nsj / nsi;
                    } else if (K->kind == LSX_COLL_CI) {                                   /* :62-70 */
                        double dE = jL->E_SI - iL->E_SI;
                        double Cup = Cv * ne[k] * exp(-dE / (KBoltzmann * T[k])) * sqrt(T[k]);
                        *Cji += Cup;
                        *Cij += Cup * nsi / nsj;
                    } else {                                                               /* CE, :88-96 */
                        double gij = iL->g / jL->g;
                        double Cdown = Cv * ne[k] * gij * sqrt(T[k]);
                        *Cij += Cdown;
                        *Cji += Cdown * nsj / nsi;
                    }
                }
                free(M);
            }
            for (size_t e = 0; e < (size_t)Nl * Nl * Ns; ++e) if (Cm[e] < 0.0) Cm[e] = 0.0;
        }
    }
    if (c->Nlines) {
        int rc = lsx_set_line_profiles(c, col0, ncol, c->aDamp + (size_t)col0 * c->Nlines * Ns, c->vBroad + (size_t)col0 * c->Natoms * Ns, s->vlos);
        if (rc) return rc;
    }
    return LSX_OK;
}

/* ---- wavelength grid, active set, the transitions' own grids ----------------------------------------
 * atomic_set.py:377-455 step by step: collect, sort, unique; searchsorted for the blue and red ends; trim a continuum at
 * its edge; membership table.  Checker for lsx_grid.cpp. */
static int cmp_double(const void* a, const void* b)
{
    double x = *(const double*)a, y = *(const double*)b;
    return (x > y) - (x < y);
}
static int32_t searchsorted_left(const double* g, int32_t n, double x)
{
    int32_t i = 0;
    while (i < n && g[i] < x) ++i;
    return i;
}
int lsx_wavelength_grid(int32_t Ntrans, const lsx_trans_grid* trans, int32_t Nextra, const double* extra,
                        double lambdaReference, int32_t capacity, double* wavelength, int32_t* Nspect,
                        int32_t* blueIdx, int32_t* redIdx)
{
    if (Ntrans < 0 || (Ntrans && !trans) || Nextra < 0 || (Nextra && !extra) || !Nspect || capacity < 0 || (capacity && !wavelength))
        return fail(LSX_EINVAL, "lsx_wavelength_grid: bad arguments");
    size_t total = (size_t)Nextra + 1;
    for (int kr = 0; kr < Ntrans; ++kr) {
        if (trans[kr].n < 1 || !trans[kr].wavelength) return fail(LSX_EINVAL, "lsx_wavelength_grid: a transition has no grid");
        for (int q = 1; q < trans[kr].n; ++q)
            if (trans[kr].wavelength[q] < trans[kr].wavelength[q - 1]) return fail(LSX_EINVAL, "lsx_wavelength_grid: a grid is not ascending");
        total += (size_t)trans[kr].n + 1;
    }
    double* g = (double*)malloc(total * sizeof(double));
    size_t m = 0;
    for (int q = 0; q < Nextra; ++q) g[m++] = extra[q];                 /* :381-383 */
    g[m++] = lambdaReference;
    for (int kr = 0; kr < Ntrans; ++kr) {                               /* :392-399 */
        const lsx_trans_grid* t = &trans[kr];
        if (t->is_line) {
            for (int q = 0; q < t->n; ++q) g[m++] = t->wavelength[q];
        } else {
            g[m++] = t->lambdaEdge;
            for (int q = 0; q < t->n; ++q) if (t->wavelength[q] <= t->lambdaEdge) g[m++] = t->wavelength[q];
        }
    }
    qsort(g, m, sizeof(double), cmp_double);                            /* :401-403 */
    size_t u = 0;
    for (size_t q = 0; q < m; ++q) if (u == 0 || g[q] != g[u - 1]) g[u++] = g[q];
    *Nspect = (int32_t)u;
    if ((size_t)capacity < u) { free(g); return fail(LSX_EINVAL, "lsx_wavelength_grid: capacity too small"); }
    memcpy(wavelength, g, u * sizeof(double));
    for (int kr = 0; kr < Ntrans; ++kr) {                               /* :407-416 */
        const lsx_trans_grid* t = &trans[kr];
        int32_t blue = searchsorted_left(g, (int32_t)u, t->wavelength[0]);
        int32_t red = searchsorted_left(g, (int32_t)u, t->wavelength[t->n - 1]) + 1;
        if (!t->is_line) {
            if (red > (int32_t)u) red = (int32_t)u;
            while (red > blue && g[red - 1] > t->lambdaEdge) red -= 1;
        }
        if (blueIdx) blueIdx[kr] = blue;
        if (redIdx) redIdx[kr] = red;
    }
    free(g);
    return LSX_OK;
}

int lsx_active_set(int32_t Ntrans, int32_t Nspect, const int32_t* blueIdx, const int32_t* redIdx, uint8_t* active)
{
    if (Ntrans < 0 || Nspect < 0 || (Ntrans && (!blueIdx || !redIdx || !active))) return fail(LSX_EINVAL, "lsx_active_set: bad arguments");
    for (int kr = 0; kr < Ntrans; ++kr) {
        if (blueIdx[kr] < 0 || redIdx[kr] > Nspect || blueIdx[kr] > redIdx[kr]) return fail(LSX_EINVAL, "lsx_active_set: range outside the grid");
        for (int la = 0; la < Nspect; ++la) active[(size_t)kr * Nspect + la] = (blueIdx[kr] <= la && la < redIdx[kr]) ? 1 : 0;   /* :434 */
    }
    return LSX_OK;
}

/* atomic_model.py:347-380 */
int lsx_line_wavelength(double lambda0, double qCore, double qWing, int32_t NlambdaGen, int32_t capacity,
                        double* wavelength, int32_t* n)
{
    if (!n || NlambdaGen < 3 || !(lambda0 > 0.0) || !(qCore > 0.0) || !(qWing > 0.0)) return fail(LSX_EINVAL, "lsx_line_wavelength: bad arguments");
    int Nlambda = (NlambdaGen % 2 == 1) ? NlambdaGen / 2 : (NlambdaGen - 1) / 2;
    Nlambda += 1;
    int NlambdaFull = 2 * Nlambda - 1;
    *n = NlambdaFull;
    if (capacity < NlambdaFull || !wavelength) return fail(LSX_EINVAL, "lsx_line_wavelength: capacity too small");
    double beta = (qWing <= 2.0 * qCore) ? 1.0 : qWing / (2.0 * qCore);
    double y = beta + sqrt(beta * beta + (beta - 1.0) * Nlambda + 2.0 - 3.0 * beta);
    double b = 2.0 * log(y) / (Nlambda - 1);
    double a = qWing / (Nlambda - 2.0 + y * y);
    double qToLambda = lambda0 * (3.0e3 / CLight);
    int Nmid = Nlambda - 1;
    wavelength[Nmid] = lambda0;
    for (int nl = 1; nl < Nlambda; ++nl) {
        double q = a * (nl + (exp(b * nl) - 1.0));
        wavelength[Nmid - nl] = lambda0 - qToLambda * q;
        wavelength[Nmid + nl] = lambda0 + qToLambda * q;
    }
    return LSX_OK;
}

/* utils.py:24-32 */
static double gaunt_bf(double wvl, double nEff, double charge)
{
    const double ERyd = 2.1798741E-18;
    double x = HC / (wvl * NM_TO_M) / (ERyd * charge * charge);
    double x3 = pow(x, 1.0 / 3.0);
    double nsqx = 1.0 / (nEff * nEff * x);
    return 1.0 + 0.1728 * x3 * (1.0 - 2.0 * nsqx) - 0.0496 * x3 * x3 * (1.0 - (1.0 - nsqx) * (2.0 / 3.0) * nsqx);
}

/* atomic_model.py:606-612 (explicit), :662-671 (hydrogenic) */
int lsx_continuum_alpha(const lsx_continuum_model* c, int32_t n, const double* wavelength, double* alpha)
{
    if (!c || n < 0 || (n && (!wavelength || !alpha))) return fail(LSX_EINVAL, "lsx_continuum_alpha: bad arguments");
    if (c->hydrogenic) {
        if (!(c->E_j > c->E_i) || c->stage_j < 1) return fail(LSX_EINVAL, "lsx_continuum_alpha: bad hydrogenic continuum");
        double Z = c->stage_j;
        double nEff = Z * sqrt(2.1798741E-18 / (c->E_j - c->E_i));
        double gbf0 = gaunt_bf(c->lambdaEdge, nEff, Z);
        for (int q = 0; q < n; ++q) {
            double gbf = gaunt_bf(wavelength[q], nEff, Z);
            alpha[q] = c->alpha0 * gbf / gbf0 * pow(wavelength[q] / c->lambdaEdge, 3.0);
            if (wavelength[q] < c->minLambda) alpha[q] = 0.0;
            if (wavelength[q] > c->lambdaEdge) alpha[q] = 0.0;
        }
        return LSX_OK;
    }
    if (c->n < 4 || c->n > 64 || !c->wavelength || !c->alpha) return fail(LSX_EINVAL, "lsx_continuum_alpha: 4 ... 64 tabulated points");
    const int m = c->n;
    const double *x = c->wavelength, *y = c->alpha;
    for (int i = 1; i < m; ++i) if (!(x[i] > x[i - 1])) return fail(LSX_EINVAL, "lsx_continuum_alpha: tabulated wavelengths must ascend strictly");
    double M[64];
    spline_moments(m, x, y, M);
    int anyneg = 0;
    for (int q = 0; q < n; ++q) {
        double w = wavelength[q], v = 0.0;
        if (w >= x[0] && w <= x[m - 1]) {
            int i = 0;
            while (i < m - 2 && w >= x[i + 1]) ++i;
            double h = x[i + 1] - x[i], aa = x[i + 1] - w, bb = w - x[i];
            v = (M[i] * aa * aa * aa + M[i + 1] * bb * bb * bb) / (6.0 * h) + (y[i] / h - M[i] * h / 6.0) * aa + (y[i + 1] / h - M[i + 1] * h / 6.0) * bb;
        }
        if (w < c->minLambda) v = 0.0;
        if (w > c->lambdaEdge) v = 0.0;
        alpha[q] = v;
        if (v < 0.0) anyneg = 1;
    }
    if (anyneg)
        for (int q = 0; q < n; ++q) {                         /* linear interp1d, fill 0, no cuts */
            double w = wavelength[q];
            if (w < x[0] || w > x[m - 1]) { alpha[q] = 0.0; continue; }
            int hi = 0;
            while (hi < m && x[hi] < w) ++hi;
            if (hi < 1) hi = 1;
            if (hi > m - 1) hi = m - 1;
            double slope = (y[hi] - y[hi - 1]) / (x[hi] - x[hi - 1]);
            alpha[q] = slope * (w - x[hi - 1]) + y[hi - 1];
        }
    return LSX_OK;
}

/* TEST HOOK (tests/envelope.py): exp(-dtau) of the short-characteristics weights moved by `g_exp_ulp` units in the last place.
 * The reference's w2 forms w1 = (1 - e) - dtau e, which cancels to dtau^2 / 2: a one-ulp difference between two correctly
 * working exponentials (numpy's SIMD exp, libm's, the GPU's table-driven one) is an ABSOLUTE 1.1e-16 on w1, up to 9e-10
 * RELATIVE just above the 5e-4 Taylor switch (formal_solver.py:36-43).  With the hook at +1 and -1 the tests measure how far
 * that moves every ray of a given problem -- the envelope inside which any faithful implementation may land -- and pin their
 * tolerances on it instead of on the last measurement.  Process-wide, 0 by default; nothing but the tests sets it. */
static int g_exp_ulp = 0;
void lsx_oracle_set_exp_ulp(int32_t n) { g_exp_ulp = n; }
static inline double exp_hooked(double x)
{
    double e = exp(x);
    if (g_exp_ulp)
        for (int i = 0; i < (g_exp_ulp > 0 ? g_exp_ulp : -g_exp_ulp); ++i) e = nextafter(e, g_exp_ulp > 0 ? 2.0 : -1.0);
    return e;
}

/* ---- formal_solver.py:14-44 ------------------------------------------------ */
static inline void w2(double dtau, double* w)
{
    if (dtau < 5e-4) {
        w[0] = dtau * (1.0 - 0.5 * dtau);
        w[1] = (dtau * dtau) * (0.5 - dtau / 3.0);
    } else if (dtau > 50.0) {
        w[0] = 1.0;
        w[1] = 1.0;
    } else {
        double expdt = exp_hooked(-dtau);
        w[0] = 1.0 - expdt;
        w[1] = w[0] - dtau * expdt;
    }
}

/* ---- formal_solver.py:46-142 ----------------------------------------------- */
static void piecewise_1d_impl(double muz, int toFrom, double Istart, int Nspace, const double* z,
                              const double* chi, const double* S, double* I, double* PsiStar)
{
    double zmu = 1.0 / muz;
    int dk, kStart, kEnd;
    if (toFrom) { dk = -1; kStart = Nspace - 1; kEnd = 0; }
    else { dk = 1; kStart = 0; kEnd = Nspace - 1; }
    double dtau_uw = 0.5 * (chi[kStart] + chi[kStart + dk]) * zmu * fabs(z[kStart] - z[kStart + dk]);
    double dS_uw = (S[kStart] - S[kStart + dk]) / dtau_uw;
    double Iupw = Istart;
    I[kStart] = Iupw;
    PsiStar[kStart] = 0.0; /* LambdaStar, divided by chi below */
    double w[2] = {0.0, 0.0};
    int k = kStart; /* the reference's loop variable survives the loop (line 138) */
    for (k = kStart + dk; k != kEnd; k += dk) {
        w2(dtau_uw, w);
        I[k] = Iupw * (1.0 - w[0]) + w[0] * S[k] + w[1] * dS_uw;
        PsiStar[k] = w[0] - w[1] / dtau_uw;
        double dtau_dw = 0.5 * (chi[k] + chi[k + dk]) * zmu * fabs(z[k] - z[k + dk]);
        double dS_dw = (S[k] - S[k + dk]) / dtau_dw;
        Iupw = I[k];
        dS_uw = dS_dw;
        dtau_uw = dtau_dw;
    }
    /* formal_solver.py:138-139: stale w and S[k] with k = kEnd - dk (reference quirk, kept) */
    int klast = kEnd - dk;
    I[kEnd] = (1.0 - w[0]) * Iupw + w[0] * S[klast] + w[1] * dS_uw;
    PsiStar[kEnd] = w[0] - w[1] / dtau_uw;
    for (int q = 0; q < Nspace; ++q) PsiStar[q] = PsiStar[q] / chi[q];
}

/* ---- N4: monotonic piecewise-parabolic short characteristics (include/lsx.h; Auer & Paletou 1994).  No counterpart
 * in the reference: parity unpinned. ---------------------------------------------------------------------------- */
static inline void w3(double dtau, double* w)
{
    if (dtau < 0.25) {
        /* w_n = sum_m (-1)^m dtau^(m+n+1) / (m! (m+n+1)), m = 0 ... 11: the closed forms below cancel to dtau^(n+1) / (n+1)
         * here (w2 would lose 5 digits at dtau = 5e-4, the switch of the linear rule's w2; at 0.25 it keeps 13) */
        double x = dtau;
        w[0] = x * (1.0 / 1.0 + x * (-1.0 / 2.0 + x * (1.0 / 6.0 + x * (-1.0 / 24.0 + x * (1.0 / 120.0 + x * (-1.0 / 720.0 + x * (1.0 / 5040.0 + x * (-1.0 / 40320.0 + x * (1.0 / 362880.0 + x * (-1.0 / 3628800.0 + x * (1.0 / 39916800.0 + x * (-1.0 / 479001600.0))))))))))));
        w[1] = x * x * (1.0 / 2.0 + x * (-1.0 / 3.0 + x * (1.0 / 8.0 + x * (-1.0 / 30.0 + x * (1.0 / 144.0 + x * (-1.0 / 840.0 + x * (1.0 / 5760.0 + x * (-1.0 / 45360.0 + x * (1.0 / 403200.0 + x * (-1.0 / 3991680.0 + x * (1.0 / 43545600.0 + x * (-1.0 / 518918400.0))))))))))));
        w[2] = x * x * x * (1.0 / 3.0 + x * (-1.0 / 4.0 + x * (1.0 / 10.0 + x * (-1.0 / 36.0 + x * (1.0 / 168.0 + x * (-1.0 / 960.0 + x * (1.0 / 6480.0 + x * (-1.0 / 50400.0 + x * (1.0 / 443520.0 + x * (-1.0 / 4354560.0 + x * (1.0 / 47174400.0 + x * (-1.0 / 558835200.0))))))))))));
    } else if (dtau > 50.0) {
        w[0] = 1.0;
        w[1] = 1.0;
        w[2] = 2.0;
    } else {
        double expdt = exp_hooked(-dtau);
        w[0] = 1.0 - expdt;
        w[1] = w[0] - dtau * expdt;
        w[2] = 2.0 * w[1] - dtau * dtau * expdt;
    }
}

static void piecewise_parabolic_1d_impl(double muz, int toFrom, double Istart, int Nspace, const double* z,
                                        const double* chi, const double* S, double* I, double* PsiStar)
{
    double zmu = 1.0 / muz;
    int dk, kStart, kEnd;
    if (toFrom) { dk = -1; kStart = Nspace - 1; kEnd = 0; }
    else { dk = 1; kStart = 0; kEnd = Nspace - 1; }
    double Iupw = Istart;
    I[kStart] = Iupw;
    PsiStar[kStart] = 0.0;
    for (int k = kStart + dk;; k += dk) {
        double w[3];
        double dtau_uw = 0.5 * (chi[k - dk] + chi[k]) * zmu * fabs(z[k - dk] - z[k]);
        double p = (S[k - dk] - S[k]) / dtau_uw;
        w3(dtau_uw, w);
        double a = p, dadS = -1.0 / dtau_uw;                          /* end point: the linear rule */
        if (k != kEnd) {
            double dtau_dw = 0.5 * (chi[k] + chi[k + dk]) * zmu * fabs(z[k] - z[k + dk]);
            double q = (S[k] - S[k + dk]) / dtau_dw;
            if (p * q > 0.0) {
                double alpha = (1.0 + dtau_dw / (dtau_uw + dtau_dw)) / 3.0, beta = 1.0 - alpha;
                double den = alpha * q + beta * p;
                a = p * q / den;
                dadS = (beta * p * p / dtau_dw - alpha * q * q / dtau_uw) / (den * den);
                if (fabs(a) > 2.0 * fabs(p)) { a = 2.0 * p; dadS = -2.0 / dtau_uw; }
            } else {
                a = 0.0;
                dadS = 0.0;
            }
        }
        double b = (p - a) / dtau_uw;
        I[k] = Iupw * (1.0 - w[0]) + w[0] * S[k] + w[1] * a + w[2] * b;
        PsiStar[k] = (w[0] + (w[1] - w[2] / dtau_uw) * dadS - w[2] / (dtau_uw * dtau_uw)) / chi[k];
        Iupw = I[k];
        if (k == kEnd) break;
    }
}

int lsx_piecewise_parabolic_1d_impl(int32_t device, int32_t nray, int32_t Nspace, const double* height, const double* mu,
                                    const int32_t* to_obs, const double* Istart, const double* chi, const double* S,
                                    double* I, double* PsiStar)
{
    (void)device;
    if (nray < 0 || Nspace < 3) return fail(LSX_EINVAL, "lsx_piecewise_parabolic_1d_impl: need Nspace >= 3");
    if (nray > 0 && (!height || !mu || !to_obs || !Istart || !chi || !S || !I || !PsiStar)) return fail(LSX_EINVAL, "lsx_piecewise_parabolic_1d_impl: null array pointer");
    for (int r = 0; r < nray; ++r)
        piecewise_parabolic_1d_impl(mu[r], to_obs[r], Istart[r], Nspace, height, chi + (size_t)r * Nspace, S + (size_t)r * Nspace,
                                    I + (size_t)r * Nspace, PsiStar + (size_t)r * Nspace);
    return LSX_OK;
}

int lsx_w3(int32_t device, int32_t n, const double* dtau, double* w)
{
    (void)device;
    if (n < 0 || (n > 0 && (!dtau || !w))) return fail(LSX_EINVAL, "lsx_w3: bad argument");
    for (int i = 0; i < n; ++i) w3(dtau[i], w + 3 * (size_t)i);
    return LSX_OK;
}

/* ---- utils.py:17-22 -------------------------------------------------------- */
static inline double planck(double temp, double wav)
{
    double hc_Tkla = HC / (KBoltzmann * NM_TO_M * wav) / temp;
    double twohnu3_c2 = (2.0 * HC) / pow(NM_TO_M * wav, 3.0);
    return twohnu3_c2 / (exp(hc_Tkla) - 1.0);
}

/* ---- formal_solver.py:144-212 ---------------------------------------------- */
static void piecewise_linear_1d(int Nspace, const double* z, const double* temperature, double muz, int toFrom,
                                double wav, const double* chi, const double* S, double* I, double* PsiStar)
{
    double zmu = 1.0 / muz;
    double Iupw;
    if (toFrom) {
        int kStart = Nspace - 1, dk = -1;
        double dtau_uw = zmu * (chi[kStart] + chi[kStart + dk]) * 0.5 * fabs(z[kStart] - z[kStart + dk]);
        double B0 = planck(temperature[Nspace - 2], wav);
        double B1 = planck(temperature[Nspace - 1], wav);
        Iupw = B1 - (B0 - B1) / dtau_uw;
    } else {
        Iupw = 0.0;
    }
    piecewise_1d_impl(muz, toFrom, Iupw, Nspace, z, chi, S, I, PsiStar);
}

int lsx_piecewise_linear_1d(int32_t device, int32_t nray, int32_t Nspace, const double* height,
                            const double* temperature, const double* mu, const int32_t* to_obs, const double* wav,
                            const double* chi, const double* S, double* I, double* PsiStar)
{
    (void)device;
    if (nray < 0 || Nspace < 3) return fail(LSX_EINVAL, "lsx_piecewise_linear_1d: need Nspace >= 3");
    for (int r = 0; r < nray; ++r)
        piecewise_linear_1d(Nspace, height, temperature, mu[r], to_obs[r], wav[r], chi + (size_t)r * Nspace,
                            S + (size_t)r * Nspace, I + (size_t)r * Nspace, PsiStar + (size_t)r * Nspace);
    return LSX_OK;
}

/* formal_solver.py:46-142 / 14-44 behind the ABI names (include/lsx.h) */
int lsx_piecewise_1d_impl(int32_t device, int32_t nray, int32_t Nspace, const double* height, const double* mu,
                          const int32_t* to_obs, const double* Istart, const double* chi, const double* S, double* I,
                          double* PsiStar)
{
    (void)device;
    if (nray < 0 || Nspace < 3) return fail(LSX_EINVAL, "lsx_piecewise_1d_impl: need Nspace >= 3");
    for (int r = 0; r < nray; ++r)
        piecewise_1d_impl(mu[r], to_obs[r], Istart[r], Nspace, height, chi + (size_t)r * Nspace, S + (size_t)r * Nspace,
                          I + (size_t)r * Nspace, PsiStar + (size_t)r * Nspace);
    return LSX_OK;
}

int lsx_w2(int32_t device, int32_t n, const double* dtau, double* w0w1)
{
    (void)device;
    if (n < 0) return fail(LSX_EINVAL, "lsx_w2: bad argument");
    for (int i = 0; i < n; ++i) w2(dtau[i], w0w1 + 2 * (size_t)i);
    return LSX_OK;
}

/* oracle-only helpers exposed for unit tests against the golden vectors */
void lsx_oracle_w2(double dtau, double* w) { w2(dtau, w); }
void lsx_oracle_piecewise_1d_impl(double muz, int32_t toFrom, double Istart, int32_t Nspace, const double* z,
                                  const double* chi, const double* S, double* I, double* PsiStar)
{
    piecewise_1d_impl(muz, toFrom, Istart, Nspace, z, chi, S, I, PsiStar);
}
double lsx_oracle_planck(double temp, double wav) { return planck(temp, wav); }

/* ---- rh_method.py:157-196 (single index form) ------------------------------- */
static double wlambda(const lsx_ctx* c, const lsx_transition* t, int lt)
{
    const double* wl = c->wavelength + t->Nblue; /* local grid == global slice (atomic_set.py:412-424) */
    double dopplerWidth = t->is_line ? CLight / t->lambda0 : 1.0;
    int N = t->Nlambda;
    if (lt == 0) return 0.5 * (wl[1] - wl[0]) * dopplerWidth;
    if (lt == N - 1) return 0.5 * (wl[N - 1] - wl[N - 2]) * dopplerWidth;
    return 0.5 * (wl[lt + 1] - wl[lt - 1]) * dopplerWidth;
}

/* ---- rh_method.py:565-708 for one column ------------------------------------ */
static void formal_sol_gamma_column(lsx_ctx* c, int col, double* scratch)
{
    const int Ns = c->Nspace, Nrays = c->Nrays, Nspect = c->Nspect;
    const double* z = c->height + (size_t)col * Ns;
    const double* T = c->temperature + (size_t)col * Ns;
    const double* n = c->n + (size_t)col * c->NLtot * Ns;
    const double* nStar = c->nStar + (size_t)col * c->NLtot * Ns;
    double* Gamma = c->Gamma + (size_t)col * c->NL2tot * Ns;
    const double* Cm = c->C + (size_t)col * c->NL2tot * Ns;
    const double* bchi = c->bg_chi + (size_t)col * Nspect * Ns;
    const double* beta = c->bg_eta + (size_t)col * Nspect * Ns;
    const double* bsca = c->bg_sca + (size_t)col * sca_per_col(c);
    const double* phi = c->phi + (size_t)col * phi_per_col(c);
    const double* wphi = c->wphi + (size_t)col * c->Nlines * Ns;
    double* J = c->J + (size_t)col * Nspect * Ns;
    double* Iout = c->I + (size_t)col * Nspect * Nrays;
    double* Rij = c->Rij + (size_t)col * c->Ntrans * Ns;
    double* Rji = c->Rji + (size_t)col * c->Ntrans * Ns;

    /* scratch carve-up */
    double* JDag = scratch;                        scratch += (size_t)Nspect * Ns;
    double* gij = scratch;                         scratch += (size_t)c->Ntrans * Ns;
    double* wla = scratch;                         scratch += (size_t)c->Ntrans * Ns;
    double* aeta = scratch;                        scratch += (size_t)c->Natoms * Ns;
    double* aU = scratch;                          scratch += (size_t)c->NLtot * Ns;
    double* achi = scratch;                        scratch += (size_t)c->NLtot * Ns;
    double* chiTot = scratch;                      scratch += Ns;
    double* etaTot = scratch;                      scratch += Ns;
    double* S = scratch;                           scratch += Ns;
    double* I = scratch;                           scratch += Ns;
    double* Psi = scratch;                         scratch += Ns;
    double* Vij = scratch;                         scratch += Ns;
    double* Vji = scratch;                         scratch += Ns;
    double* Uji = scratch;                         scratch += Ns;
    double* Ieff = scratch;                        scratch += Ns;

    /* :587-590  Gamma = 0 + C */
    for (size_t q = 0; q < (size_t)c->NL2tot * Ns; ++q) Gamma[q] = 0.0 + Cm[q];
    /* :592-593 */
    memcpy(JDag, J, (size_t)Nspect * Ns * 8);
    memset(J, 0, (size_t)Nspect * Ns * 8);

    const double hc_k = HC / (KBoltzmann * NM_TO_M);
    const double hc_4pi = 0.25 * HC / M_PI;

    for (int la = 0; la < Nspect; ++la) {
        const double wav = c->wavelength[la];
        /* setup_wavelength, :425-455 */
        memset(gij, 0, (size_t)c->Ntrans * Ns * 8);
        memset(wla, 0, (size_t)c->Ntrans * Ns * 8);
        for (int kr = 0; kr < c->Ntrans; ++kr) {
            const lsx_transition* t = &c->trans[kr];
            if (!c->active[(size_t)kr * Nspect + la]) continue;
            int lt = la - t->Nblue;
            double wl = wlambda(c, t, lt);
            if (t->is_line) {
                const double* wp = wphi + (size_t)c->line_idx[kr] * Ns;
                for (int k = 0; k < Ns; ++k) {
                    gij[kr * Ns + k] = t->Bji / t->Bij;
                    wla[kr * Ns + k] = wl * wp[k] / HC;
                }
            } else {
                const double* nsi = nStar + (size_t)(c->lev_off[t->atom] + t->i) * Ns;
                const double* nsj = nStar + (size_t)(c->lev_off[t->atom] + t->j) * Ns;
                for (int k = 0; k < Ns; ++k) {
                    gij[kr * Ns + k] = nsi[k] / nsj[k] * exp(-hc_k / wav / T[k]);
                    wla[kr * Ns + k] = wl / wav / HPlanck;
                }
            }
        }
        for (int mu = 0; mu < Nrays; ++mu) {
            for (int toFrom = 0; toFrom < 2; ++toFrom) {
                memset(chiTot, 0, Ns * 8);
                memset(etaTot, 0, Ns * 8);
                memset(aeta, 0, (size_t)c->Natoms * Ns * 8);
                memset(aU, 0, (size_t)c->NLtot * Ns * 8);
                memset(achi, 0, (size_t)c->NLtot * Ns * 8);
                for (int kr = 0; kr < c->Ntrans; ++kr) {
                    const lsx_transition* t = &c->trans[kr];
                    if (!c->active[(size_t)kr * Nspect + la]) continue;
                    int lt = la - t->Nblue;
                    const double* ni = n + (size_t)(c->lev_off[t->atom] + t->i) * Ns;
                    const double* nj = n + (size_t)(c->lev_off[t->atom] + t->j) * Ns;
                    double* chi_i = achi + (size_t)(c->lev_off[t->atom] + t->i) * Ns;
                    double* chi_j = achi + (size_t)(c->lev_off[t->atom] + t->j) * Ns;
                    double* U_j = aU + (size_t)(c->lev_off[t->atom] + t->j) * Ns;
                    double* eta_a = aeta + (size_t)t->atom * Ns;
                    /* uv(), :245-288 */
                    if (t->is_line) {
                        const double* ph = c->phi_compact
                            ? phi + ((size_t)c->phi_off[kr] + lt) * Ns
                            : phi + ((((size_t)c->phi_off[kr] + lt) * Nrays + mu) * 2 + toFrom) * Ns;
                        double AB = t->Aji / t->Bji;
                        double hB = hc_4pi * t->Bij;
                        for (int k = 0; k < Ns; ++k) {
                            Vij[k] = hB * ph[k];
                            Vji[k] = gij[kr * Ns + k] * Vij[k];
                            Uji[k] = AB * Vji[k];
                        }
                    } else {
                        double al = c->alpha[c->alpha_off[kr] + lt];
                        double f = 2.0 * HC / pow(NM_TO_M * wav, 3.0);
                        for (int k = 0; k < Ns; ++k) {
                            Vij[k] = al;
                            Vji[k] = gij[kr * Ns + k] * Vij[k];
                            Uji[k] = f * Vji[k];
                        }
                    }
                    for (int k = 0; k < Ns; ++k) { /* :613-627 */
                        double chi = ni[k] * Vij[k] - nj[k] * Vji[k];
                        double eta = nj[k] * Uji[k];
                        chi_i[k] += chi;
                        chi_j[k] -= chi;
                        U_j[k] += Uji[k];
                        chiTot[k] += chi;
                        etaTot[k] += eta;
                        eta_a[k] += eta;
                    }
                }
                const double* sca = bsca + (c->sca_per_lambda ? (size_t)la * Ns : 0);
                for (int k = 0; k < Ns; ++k) { /* :630-632 */
                    chiTot[k] += bchi[(size_t)la * Ns + k];
                    S[k] = (etaTot[k] + beta[(size_t)la * Ns + k] + sca[k] * JDag[(size_t)la * Ns + k]) / chiTot[k];
                }
                if (c->solver == LSX_SOLVER_PARABOLIC) {   /* N4: same boundary condition (formal_solver.py:203-209), parabolic rule */
                    double Istart = 0.0;
                    if (toFrom) {
                        double dtau_uw = (1.0 / c->muz[mu]) * (chiTot[Ns - 1] + chiTot[Ns - 2]) * 0.5 * fabs(z[Ns - 1] - z[Ns - 2]);
                        double B0 = planck(T[Ns - 2], wav), B1 = planck(T[Ns - 1], wav);
                        Istart = B1 - (B0 - B1) / dtau_uw;
                    }
                    piecewise_parabolic_1d_impl(c->muz[mu], toFrom, Istart, Ns, z, chiTot, S, I, Psi);
                } else
                piecewise_linear_1d(Ns, z, T, c->muz[mu], toFrom, wav, chiTot, S, I, Psi); /* :635 */
                Iout[(size_t)la * Nrays + mu] = I[0];                                    /* :638 */
                double hw = 0.5 * c->wmu[mu];
                for (int k = 0; k < Ns; ++k) J[(size_t)la * Ns + k] += hw * I[k];        /* :640 */

                for (int a = 0; a < c->Natoms; ++a) { /* :643-692 */
                    for (int k = 0; k < Ns; ++k) Ieff[k] = I[k] - Psi[k] * aeta[(size_t)a * Ns + k];
                    for (int kr = 0; kr < c->Ntrans; ++kr) {
                        const lsx_transition* t = &c->trans[kr];
                        if (t->atom != a || !c->active[(size_t)kr * Nspect + la]) continue;
                        int lt = la - t->Nblue;
                        if (t->is_line) {
                            const double* ph = c->phi_compact
                                ? phi + ((size_t)c->phi_off[kr] + lt) * Ns
                                : phi + ((((size_t)c->phi_off[kr] + lt) * Nrays + mu) * 2 + toFrom) * Ns;
                            double AB = t->Aji / t->Bji;
                            double hB = hc_4pi * t->Bij;
                            for (int k = 0; k < Ns; ++k) {
                                Vij[k] = hB * ph[k];
                                Vji[k] = gij[kr * Ns + k] * Vij[k];
                                Uji[k] = AB * Vji[k];
                            }
                        } else {
                            double al = c->alpha[c->alpha_off[kr] + lt];
                            double f = 2.0 * HC / pow(NM_TO_M * wav, 3.0);
                            for (int k = 0; k < Ns; ++k) {
                                Vij[k] = al;
                                Vji[k] = gij[kr * Ns + k] * Vij[k];
                                Uji[k] = f * Vji[k];
                            }
                        }
                        const int Nl = c->Nlevel[a];
                        double* G = Gamma + (size_t)c->lev2_off[a] * Ns;
                        double* Gij = G + ((size_t)t->i * Nl + t->j) * Ns;
                        double* Gji = G + ((size_t)t->j * Nl + t->i) * Ns;
                        const double* chi_i = achi + (size_t)(c->lev_off[a] + t->i) * Ns;
                        const double* chi_j = achi + (size_t)(c->lev_off[a] + t->j) * Ns;
                        const double* U_i = aU + (size_t)(c->lev_off[a] + t->i) * Ns;
                        const double* U_j = aU + (size_t)(c->lev_off[a] + t->j) * Ns;
                        for (int k = 0; k < Ns; ++k) {
                            double wlamu = wla[kr * Ns + k] * hw * 4 * M_PI;
                            double integrand = (Uji[k] + Vji[k] * Ieff[k]) - (chi_i[k] * Psi[k] * U_j[k]);
                            Gij[k] += integrand * wlamu;
                            integrand = (Vij[k] * Ieff[k]) - (chi_j[k] * Psi[k] * U_i[k]);
                            Gji[k] += integrand * wlamu;
                            /* :691-692 (quirk kept: Vij in Rji, never zeroed between calls) */
                            Rij[(size_t)kr * Ns + k] += I[k] * Vij[k] * wlamu;
                            Rji[(size_t)kr * Ns + k] += (Uji[k] + I[k] * Vij[k]) * wlamu;
                        }
                    }
                }
            }
        }
    }
    /* :698-703 diagonal */
    for (int a = 0; a < c->Natoms; ++a) {
        const int Nl = c->Nlevel[a];
        double* G = Gamma + (size_t)c->lev2_off[a] * Ns;
        for (int k = 0; k < Ns; ++k) {
            for (int i = 0; i < Nl; ++i) G[((size_t)i * Nl + i) * Ns + k] = 0.0;
            for (int i = 0; i < Nl; ++i) {
                double s = 0.0;
                for (int l = 0; l < Nl; ++l) s += G[((size_t)l * Nl + i) * Ns + k];
                G[((size_t)i * Nl + i) * Ns + k] = -s;
            }
        }
    }
    /* :705-706 */
    double dJ = 0.0;
    int nan = 0;
    for (size_t q = 0; q < (size_t)Nspect * Ns; ++q) {
        double v = fabs(1.0 - JDag[q] / J[q]);
        if (v != v) nan = 1;
        else if (v > dJ) dJ = v;
    }
    c->dJcol[col] = nan ? NAN : dJ;
}

static size_t fs_scratch_doubles(const lsx_ctx* c)
{
    size_t Ns = c->Nspace;
    return (size_t)c->Nspect * Ns + 2 * (size_t)c->Ntrans * Ns + (size_t)c->Natoms * Ns + 2 * (size_t)c->NLtot * Ns + 9 * Ns;
}

static double colmax(const double* v, int n)
{
    double m = 0.0;
    for (int i = 0; i < n; ++i) {
        if (v[i] != v[i]) return NAN;
        if (v[i] > m) m = v[i];
    }
    return m;
}

int lsx_formal_sol_gamma_async(lsx_ctx* c)
{
    if (!c) return fail(LSX_EINVAL, "null ctx");
    c->spec_valid = 0;
    size_t nd = fs_scratch_doubles(c);
#ifdef _OPENMP
#pragma omp parallel num_threads(c->nthreads)
#endif
    {
        double* scratch = (double*)malloc(nd * 8);
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 1)
#endif
        for (int col = 0; col < c->ncol; ++col) {
            if (c->colmask && !c->colmask[col]) { c->dJcol[col] = 0.0; continue; }
            formal_sol_gamma_column(c, col, scratch);
        }
        free(scratch);
    }
    c->last_dJ = colmax(c->dJcol, c->ncol);
    return LSX_OK;
}

int lsx_formal_sol_gamma(lsx_ctx* c, double* dJ)
{
    int rc = lsx_formal_sol_gamma_async(c);
    if (rc) return rc;
    if (dJ) *dJ = c->last_dJ;
    return LSX_OK;
}

/* The pipelined-loop entries of the ABI (include/lsx.h).  The oracle computes synchronously, so a speculative formal solution
 * simply keeps a copy of everything the call overwrites (J, I, Gamma, the accumulated Rij / Rji, the per-column dJ) and
 * lsx_discard_formal_sol puts it back; lsx_sync_begin has nothing to enqueue and lsx_sync_end is lsx_sync. */
static void spec_copy(lsx_ctx* c, int restore)
{
    const size_t nc = (size_t)c->ncol, Ns = (size_t)c->Nspace;
    const size_t nt = (size_t)(c->Ntrans ? c->Ntrans : 1);
    double* arr[6] = {c->J, c->I, c->Gamma, c->Rij, c->Rji, c->dJcol};
    const size_t len[6] = {nc * c->Nspect * Ns, nc * c->Nspect * c->Nrays, nc * c->NL2tot * Ns, nc * nt * Ns, nc * nt * Ns, nc};
    size_t tot = 0;
    for (int i = 0; i < 6; ++i) tot += len[i];
    if (!c->spec_save) c->spec_save = (double*)malloc(tot * 8);
    double* q = c->spec_save;
    for (int i = 0; i < 6; ++i) {
        if (restore) memcpy(arr[i], q, len[i] * 8);
        else memcpy(q, arr[i], len[i] * 8);
        q += len[i];
    }
}

int lsx_formal_sol_gamma_speculative(lsx_ctx* c)
{
    if (!c) return fail(LSX_EINVAL, "null ctx");
    if (c->colmask) return fail(LSX_EUNSUPPORTED, "lsx_formal_sol_gamma_speculative: not with frozen columns (lsx_set_active_columns)");
    spec_copy(c, 0);
    c->spec_last_dJ = c->last_dJ;
    int rc = lsx_formal_sol_gamma_async(c);
    c->spec_valid = rc == LSX_OK;
    return rc;
}

int lsx_discard_formal_sol(lsx_ctx* c)
{
    if (!c) return fail(LSX_EINVAL, "null ctx");
    if (!c->spec_valid) return fail(LSX_EINVAL, "lsx_discard_formal_sol: the last call was not a speculative formal solution");
    if (c->mon_set && c->mon_spec)
        return fail(LSX_EINVAL, "lsx_discard_formal_sol: a read-back begun after the speculative call is in flight (lsx_sync_end first: "
                                "it would report the discarded call's monitors)");
    spec_copy(c, 1);
    c->last_dJ = c->spec_last_dJ;
    c->spec_valid = 0;
    return LSX_OK;
}

int lsx_prefers_lookahead(lsx_ctx* c)
{
    (void)c;
    return 0;
}

int lsx_sync_begin(lsx_ctx* c)
{
    if (!c) return fail(LSX_EINVAL, "null ctx");
    if (c->mon_set) return fail(LSX_EINVAL, "lsx_sync_begin: the previous read-back has not been collected (lsx_sync_end)");
    c->mon_dJ = c->last_dJ;
    c->mon_dP = c->last_dP;
    c->mon_set = 1;
    c->mon_spec = c->spec_valid;      /* (as the HIP library: collect this read-back before discarding the call it reports) */
    c->mon_n_pending = c->mon_n_valid = 0;
    return LSX_OK;
}

/* include/lsx.h: the read-back that also brings the populations (the drop-in Context's stat_equil, rh_method.py:412-416, 736-741).
 * Synchronous here: a snapshot. */
int lsx_sync_begin_populations(lsx_ctx* c)
{
    int rc = lsx_sync_begin(c);
    if (rc) return rc;
    const size_t nb = (size_t)c->ncol * c->NLtot * c->Nspace * sizeof(double);
    if (!c->mon_n) c->mon_n = (double*)malloc(nb);
    if (!c->mon_n) return fail(LSX_EINVAL, "lsx_sync_begin_populations: out of memory");
    memcpy(c->mon_n, c->n, nb);
    c->mon_n_pending = 1;
    return LSX_OK;
}

int lsx_fetch_populations(lsx_ctx* c, double* dst, size_t nbytes)
{
    if (!c || !dst) return fail(LSX_EINVAL, "lsx_fetch_populations: null argument");
    if (!c->mon_n_valid) return fail(LSX_EINVAL, "lsx_fetch_populations: no collected read-back of the populations (lsx_sync_begin_populations, lsx_sync_end)");
    if (nbytes != (size_t)c->ncol * c->NLtot * c->Nspace * sizeof(double)) return fail(LSX_EINVAL, "lsx_fetch_populations: nbytes does not match [ncol][NLtot][Nspace]");
    memcpy(dst, c->mon_n, nbytes);
    return LSX_OK;
}

/* dense solve A x = b, A column-major N x N, LU with partial pivoting in the order
 * of LAPACK dgetf2 + dgetrs (what scipy.linalg.solve -> dgesv does, rh_method.py:739).
 * returns 0 ok, 1 singular or not finite. */
static int gesv(int N, double* A, double* b)
{
    for (int j = 0; j < N; ++j) {
        int p = j;
        double amax = fabs(A[j + j * N]);
        for (int i = j + 1; i < N; ++i) {
            double v = fabs(A[i + j * N]);
            if (v > amax) { amax = v; p = i; }
        }
        if (A[p + j * N] == 0.0 || amax != amax) return 1; /* a NaN anywhere ends on a diagonal: the system is refused like a singular
                                                             * one (scipy.linalg.solve refuses it too: check_finite) */
        if (p != j) {
            for (int q = 0; q < N; ++q) { double t = A[j + q * N]; A[j + q * N] = A[p + q * N]; A[p + q * N] = t; }
            double t = b[j]; b[j] = b[p]; b[p] = t;
        }
        double r = 1.0 / A[j + j * N];
        for (int i = j + 1; i < N; ++i) A[i + j * N] *= r;
        for (int q = j + 1; q < N; ++q) {
            double ajq = A[j + q * N];
            for (int i = j + 1; i < N; ++i) A[i + q * N] -= A[i + j * N] * ajq;
        }
    }
    for (int j = 0; j < N; ++j) /* L y = b */
        for (int i = j + 1; i < N; ++i) b[i] -= A[i + j * N] * b[j];
    for (int j = N - 1; j >= 0; --j) { /* U x = y */
        b[j] /= A[j + j * N];
        for (int i = 0; i < j; ++i) b[i] -= A[i + j * N] * b[j];
    }
    return 0;
}

/* ---- rh_method.py:710-745 for one column ----------------------------------- */
static int stat_equil_column(lsx_ctx* c, int col)
{
    const int Ns = c->Nspace;
    double maxRel = 0.0;
    int singular = 0;
    double A[32 * 32], b[32], nOld[32];
    for (int a = 0; a < c->Natoms; ++a) {
        const int Nl = c->Nlevel[a];
        double* n = c->n + ((size_t)col * c->NLtot + c->lev_off[a]) * Ns;
        const double* G = c->Gamma + ((size_t)col * c->NL2tot + c->lev2_off[a]) * Ns;
        const double* nTot = c->nTotal + ((size_t)col * c->Natoms + a) * Ns;
        for (int k = 0; k < Ns; ++k) {
            int iE = 0; /* np.argmax: first maximum */
            for (int l = 1; l < Nl; ++l)
                if (n[(size_t)l * Ns + k] > n[(size_t)iE * Ns + k]) iE = l;
            for (int i = 0; i < Nl; ++i)
                for (int j = 0; j < Nl; ++j) A[i + j * Nl] = (i == iE) ? 1.0 : G[((size_t)i * Nl + j) * Ns + k];
            for (int i = 0; i < Nl; ++i) { b[i] = 0.0; nOld[i] = n[(size_t)i * Ns + k]; }
            b[iE] = nTot[k];
            if (gesv(Nl, A, b)) {
                if (!singular) { singular = 1; c->sing_col[col] = ((long)k << 8) | a; }
                continue;
            }
            /* change.max() is numpy's max: NaN wins among the levels of this depth; the running
             * maxRelChange = max(maxRelChange, change.max()) is Python's builtin max, which keeps
             * maxRelChange when the new value is NaN (rh_method.py:740-741) */
            double chmax = 0.0;
            int nan = 0;
            for (int i = 0; i < Nl; ++i) {
                double ch = fabs(1.0 - nOld[i] / b[i]);
                if (ch != ch) nan = 1;
                else if (ch > chmax) chmax = ch;
                n[(size_t)i * Ns + k] = b[i];
            }
            if (!nan && chmax > maxRel) maxRel = chmax;
        }
    }
    c->dPcol[col] = maxRel;
    return singular;
}

int lsx_stat_equil_async(lsx_ctx* c)
{
    if (!c) return fail(LSX_EINVAL, "null ctx");
    c->spec_valid = 0;
    for (int a = 0; a < c->Natoms; ++a)
        if (c->Nlevel[a] > 32) return fail(LSX_EUNSUPPORTED, "oracle stat_equil: Nlevel > 32");
    int sing = 0;
#ifdef _OPENMP
#pragma omp parallel for num_threads(c->nthreads) reduction(| : sing)
#endif
    for (int col = 0; col < c->ncol; ++col) {
        c->sing_col[col] = -1;
        if (c->colmask && !c->colmask[col]) { c->dPcol[col] = 0.0; continue; }
        sing |= stat_equil_column(c, col);
    }
    c->last_dP = colmax(c->dPcol, c->ncol);
    if (sing) {
        char msg[256];
        int col = 0;
        while (col < c->ncol && c->sing_col[col] < 0) ++col;
        snprintf(msg, sizeof msg, "stat_equil: singular matrix at column %d, depth %ld, atom %ld (the first such system; cf. "
                                  "LinAlgError at rh_method.py:739)", col, c->sing_col[col] >> 8, c->sing_col[col] & 0xff);
        return fail(LSX_ESINGULAR, msg);
    }
    return LSX_OK;
}

int lsx_stat_equil(lsx_ctx* c, double* dP)
{
    int rc = lsx_stat_equil_async(c);
    if (rc) return rc;
    if (dP) *dP = c->last_dP;
    return LSX_OK;
}

int lsx_set_formal_solver(lsx_ctx* c, int32_t solver)
{
    if (!c || (solver != LSX_SOLVER_LINEAR && solver != LSX_SOLVER_PARABOLIC)) return fail(LSX_EINVAL, "lsx_set_formal_solver: bad argument");
    c->solver = solver;
    return LSX_OK;
}

/* include/lsx.h: the choice between the HIP library's two wavefront mappings.  The oracle has one code path: it checks the
 * arguments like the HIP library does and changes nothing. */
int lsx_set_sweep_policy(lsx_ctx* c, int32_t policy, int32_t decide_for_columns)
{
    if (!c || policy < LSX_SWEEP_AUTO || policy > LSX_SWEEP_RAY_SERIAL || decide_for_columns < 0)
        return fail(LSX_EINVAL, "lsx_set_sweep_policy: bad argument");
    return LSX_OK;
}

int32_t lsx_sweep_policy(const lsx_ctx* c)
{
    (void)c;
    return 0;
}

/* include/lsx.h, explicit options: the oracle has ONE code path, so a well-formed list is accepted and ignored */
int lsx_create_with_options(const lsx_problem* d, int32_t ncol, int32_t device, void* stream, const char* options, lsx_ctx** out)
{
    if (options) {
        const char* p = options;
        while (*p) {                                   /* key=value(,|;)... : every entry needs a '=' with text on both sides */
            const char* e = p;
            while (*e && *e != ',' && *e != ';') ++e;
            const char* q = p;
            while (q < e && *q != '=') ++q;
            int blank = 1;
            for (const char* t = p; t < e; ++t) if (*t != ' ') blank = 0;
            if (!blank && (q == p || q >= e - 1)) return fail(LSX_EINVAL, "lsx_create_with_options: expected key=value");
            p = *e ? e + 1 : e;
        }
    }
    return lsx_create(d, ncol, device, stream, out);
}

int lsx_effective_options(const lsx_ctx* c, char* buf, size_t n)
{
    static const char kWhat[] = "backend=oracle-c";
    if (!c || !buf || n < sizeof kWhat) return fail(LSX_EINVAL, "lsx_effective_options: bad argument");
    memcpy(buf, kWhat, sizeof kWhat);
    return LSX_OK;
}

uint64_t lsx_options_signature(const lsx_ctx* c)
{
    static const char kWhat[] = "backend=oracle-c";
    uint64_t h = 0xcbf29ce484222325ull;                /* FNV-1a, as the HIP library hashes its own string */
    if (!c) return 0;
    for (const char* p = kWhat; *p; ++p) { h ^= (unsigned char)*p; h *= 0x100000001b3ull; }
    return h;
}

int lsx_set_active_columns(lsx_ctx* c, const uint8_t* active)
{
    if (!c) return fail(LSX_EINVAL, "null ctx");
    free(c->colmask);
    c->colmask = NULL;
    if (active) {
        c->colmask = (uint8_t*)malloc((size_t)c->ncol);
        memcpy(c->colmask, active, (size_t)c->ncol);
    }
    return LSX_OK;
}

int lsx_sync(lsx_ctx* c, double* dJ, double* dP)
{
    if (!c) return fail(LSX_EINVAL, "null ctx");
    if (c->mon_set) { c->mon_n_valid = c->mon_n_pending; c->mon_n_pending = 0; }
    c->mon_set = 0;
    if (dJ) *dJ = c->last_dJ;
    if (dP) *dP = c->last_dP;
    return LSX_OK;
}

int lsx_sync_end(lsx_ctx* c, double* dJ, double* dP)
{
    if (!c) return fail(LSX_EINVAL, "null ctx");
    if (!c->mon_set) return lsx_sync(c, dJ, dP);
    c->mon_set = 0;
    c->mon_n_valid = c->mon_n_pending; c->mon_n_pending = 0;
    if (dJ) *dJ = c->mon_dJ;
    if (dP) *dP = c->mon_dP;
    return LSX_OK;
}

int lsx_monitors(lsx_ctx* c, double* dst)
{
    if (!c || !dst) return fail(LSX_EINVAL, "lsx_monitors: null argument");
    double mj = 0.0, mp = 0.0, nan = 0.0, sing = 0.0;
    for (int col = 0; col < c->ncol; ++col) {
        if (c->dJcol[col] != c->dJcol[col]) nan = 1.0;
        else if (c->dJcol[col] > mj) mj = c->dJcol[col];
        if (c->dPcol[col] > mp) mp = c->dPcol[col];
        if (c->sing_col[col] >= 0) sing = 1.0;
    }
    dst[0] = mj; dst[1] = mp; dst[2] = nan; dst[3] = sing;
    return LSX_OK;
}

static int locate(lsx_ctx* c, int what, double** base, size_t* per)
{
    size_t Ns = c->Nspace;
    switch (what) {
    case LSX_I: *base = c->I; *per = (size_t)c->Nspect * c->Nrays; break;
    case LSX_J: *base = c->J; *per = (size_t)c->Nspect * Ns; break;
    case LSX_N: *base = c->n; *per = (size_t)c->NLtot * Ns; break;
    case LSX_GAMMA: *base = c->Gamma; *per = (size_t)c->NL2tot * Ns; break;
    case LSX_DJ_COL: *base = c->dJcol; *per = 1; break;
    case LSX_DPOPS_COL: *base = c->dPcol; *per = 1; break;
    case LSX_NSTAR: *base = c->nStar; *per = (size_t)c->NLtot * Ns; break;
    case LSX_C: *base = c->C; *per = (size_t)c->NL2tot * Ns; break;
    case LSX_PHI: *base = c->phi; *per = phi_per_col(c); break;
    case LSX_WPHI: *base = c->wphi; *per = (size_t)c->Nlines * Ns; break;
    case LSX_VBROAD: *base = c->vBroad; *per = (size_t)c->Natoms * Ns; if (!c->vBroad) return 1; break;
    case LSX_ADAMP: *base = c->aDamp; *per = (size_t)(c->Nlines ? c->Nlines : 1) * Ns; if (!c->aDamp) return 1; break;
    default: return 1;
    }
    return 0;
}

int lsx_get(lsx_ctx* c, int32_t what, int32_t col0, int32_t ncol, double* dst, size_t nbytes)
{
    double* base; size_t per;
    if (!c || !dst || col0 < 0 || ncol < 1 || col0 + ncol > c->ncol) return fail(LSX_EINVAL, "lsx_get: bad range");
    if (locate(c, what, &base, &per)) return fail(LSX_EINVAL, "lsx_get: unknown item");
    if (nbytes != per * ncol * 8) return fail(LSX_EINVAL, "lsx_get: nbytes does not match the item's shape");
    memcpy(dst, base + per * col0, nbytes);
    return LSX_OK;
}

int lsx_set(lsx_ctx* c, int32_t what, int32_t col0, int32_t ncol, const double* src, size_t nbytes)
{
    double* base; size_t per;
    if (!c || !src || col0 < 0 || ncol < 1 || col0 + ncol > c->ncol) return fail(LSX_EINVAL, "lsx_set: bad range");
    if (what != LSX_N && what != LSX_J) return fail(LSX_EINVAL, "lsx_set: only LSX_N and LSX_J are writable");
    locate(c, what, &base, &per);
    if (nbytes != per * ncol * 8) return fail(LSX_EINVAL, "lsx_set: nbytes does not match the item's shape");
    memcpy(base + per * col0, src, nbytes);
    return LSX_OK;
}

#include <time.h>
int lsx_time_formal_sol(lsx_ctx* c, int32_t warmup, int32_t reps, double* ms_total, double* ms_sweep)
{
    if (!c || reps < 1) return fail(LSX_EINVAL, "lsx_time_formal_sol: bad argument");
    for (int i = 0; i < warmup; ++i) lsx_formal_sol_gamma_async(c);
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int i = 0; i < reps; ++i) lsx_formal_sol_gamma_async(c);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    double ms = ((t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6) / reps;
    if (ms_total) *ms_total = ms;
    if (ms_sweep) *ms_sweep = ms;
    return LSX_OK;
}

/* B_alg = 8 Ns [P SNl + 2 Nspect (bg) + 2 Nspect (Jdag, J) + 1 (sigma) + NLtot (n)
 *                          + 2 NL2tot (C, Gamma) + 6] + 8 Nspect Nrays */
double lsx_algorithmic_bytes_per_column(const lsx_ctx* c)
{
    double P = c->phi_compact ? 1.0 : 2.0 * c->Nrays;
    double per_depth = P * c->SNl + 4.0 * c->Nspect + (c->sca_per_lambda ? c->Nspect : 1.0) + c->NLtot + 2.0 * c->NL2tot + 6.0;
    return 8.0 * c->Nspace * per_depth + 8.0 * c->Nspect * c->Nrays;
}
