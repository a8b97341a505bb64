/* lsx_hip_background.h -- the background of a column on the device: the Wittmann equation of state and the ATLAS-style
 * continuous opacity the reference evaluates in Background(atmos, spect) (background.py:15-53, witt.py); an entry of the HIP
 * library alone, included by lsx_hip.h.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays; everything is
 * checked on the host before anything is launched. */
#ifndef LSX_HIP_BACKGROUND_H
#define LSX_HIP_BACKGROUND_H

#include "lsx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The partition functions and abundances the equation of state works from.  The library reads no file: the caller hands over
 * what witt.init_pf_data reads from the Kurucz table (lightspinner_amd.background.EosTables.from_kurucz_xdr parses it). */
typedef struct lsx_eos_tables {
    int32_t npf;            /* points of the temperature grid (201 in pf_Kurucz.input)                                  */
    int32_t nelem;          /* elements given, H first, by atomic number; >= 28 (witt.ncontr)                           */
    const double* tpf;      /* [npf] K, strictly ascending                                                              */
    const int32_t* nstage;  /* [nelem], 1..6                                                                            */
    const double* pf;       /* [nelem][6][npf], stages beyond nstage not read                                           */
    const double* eion;     /* [nelem][6] eV, as witt.init_pf_data(to_EV=True) leaves them                              */
    const double* abund;    /* [99] as read, NOT normalised; the library normalises (witt.py:166-176)                   */
    const double* amass;    /* [99] amu                                                                                 */
    double weight_per_H;    /* atomicTable.weightPerH (background.py:32)                                                */
    int32_t iter_cap;       /* 0: the reference's caps (below); > 0: every EOS loop stops after this many passes        */
    int32_t reserved;
} lsx_eos_tables;

/* The equation of state alone, for ncol columns of the context's Nspace depths: rho = Amu weightPerH nHTot CM_TO_M^3 / G_TO_KG,
 * pgas = witt.pg_from_rho(T, rho), pe = witt.pe_from_rho(T, rho) (two separate solves, background.py:33-35) and the 17 partial
 * densities of witt.getBackgroundPartials(T, pgas, pe, divide_by_u=True).
 *   temperature, nHTot: [ncol][Nspace], SI (as after Atmosphere.nondimensionalise).
 *   pgas, pe: [ncol][Nspace], dyn cm^-2; partials: [ncol][17][Nspace]; status: int32 [ncol][Nspace], the number of witt.pe_pg
 *   evaluations the point took, negated where a loop ran to its cap (also if its last pass met the stop test).  Any output
 *   pointer may be NULL.
 * Caps: witt.pe_from_pg 250 and witt.pg_from_rho 100 as in the reference; witt.pe_from_rho, whose counter the reference never
 * increments (witt.py:268-277), 250 here.  tab->iter_cap > 0 replaces all three.  A point that hits a cap makes the call return
 * LSX_ENOCONV (the message names the first column and depth); the outputs are still written.
 * ctx supplies Nspace, the device and the stream; the call does not touch the context's state.
 * abtot, ab_others, avw, muH and rho_from_H are formed on the host as sequential sums (numpy sums pairwise: they may differ from
 * the reference's by a few units in the last place). */
int lsx_hip_eos(lsx_ctx* ctx, const lsx_eos_tables* tab, int32_t ncol, const double* temperature, const double* nHTot,
                double* pgas, double* pe, double* partials, int32_t* status);

/* The background of ncol columns: chi = witt.contOpacity(T, pgas, pe, 10 lambda) / CM_TO_M (the sum A + B of witt.cop, with its
 * switches at 12 000 K and 30 000 K), eta = planck(T, lambda) chi, sca = ne sigma_Thomson (background.py:10-13).
 *   temperature, nHTot, ne: [ncol][Nspace], SI.
 *   wavelength != NULL: nla wavelengths in nm, strictly ascending, finite, > 0.  chi, eta: [ncol][nla][Nspace]; sca:
 *     [ncol][Nspace]; host memory, the layout lsx_hip_spectrum takes as bg_chi / bg_eta.  install must be 0.
 *   wavelength == NULL: the context's own grid (nla is not read).  install = 1 puts the result into the context as the background
 *     of columns [col0, col0 + ncol) (col0 is read only then; without install any ncol >= 1 is computed), through the steps
 *     lsx_set_columns takes for bg_chi / bg_eta / bg_sca (on a sca_per_lambda context the Thomson value is broadcast over
 *     wavelength); any of chi, eta, sca may then be NULL.  It invalidates what
 *     lsx_set_columns invalidates for a new background and nothing else: populations, J, profiles and Ng state keep their bits.
 *     The columns must have been set before (geometry and temperature come from lsx_set_columns).
 * LSX_ENOCONV (a point of the equation of state hit a cap): nothing is installed for any column of the call.
 * LSX_EINVAL: non-finite or non-positive temperature, nHTot, ne; nelem < 28, a non-ascending tpf, an nstage outside 1..6, an
 * element the opacity needs (H, He, C, N, O, Mg, Al, Si, Ca, Fe) with fewer stages than getBackgroundPartials reads; a bad
 * column range; bad wavelengths; install with wavelength != NULL; install on a context whose columns were never set. */
int lsx_hip_background(lsx_ctx* ctx, const lsx_eos_tables* tab, int32_t col0, int32_t ncol, const double* temperature,
                       const double* nHTot, const double* ne, int32_t nla, const double* wavelength, double* chi, double* eta,
                       double* sca, int32_t install);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_BACKGROUND_H */
