// lsx_scales_dev.h -- the depth-scale conversion of AtmosphereConstructor.convert_scales (atmosphere.py:81-141), restated as
// __host__ __device__ functions that a host compiler also accepts (lsx_background.hip runs them on the device, one lane per
// column; lsx_scales_host.cpp on the CPU for the tests).  The reference's operation order is kept expression by expression (C and
// Python associate + - * / alike; build with -ffp-contract=off).  The recurrences need the previous depth only: Run carries it.
#pragma once
#include "lsx_background_dev.h"

namespace lsxsc {

enum { GEOMETRIC = 0, COLUMN_MASS = 1, TAU500 = 2 };      // ScaleType (atmosphere.py:13-16), LSX_SCALE_*
constexpr double KBOLTZMANN = 1.380658E-23;                // constants.py:4

// rhoSI = Const.Amu * atomicTable.weightPerH * self.nHTot (:81); amu_wph = Amu * weightPerH (EosParams::rho_unit)
LSXBG_HD double rho_si(double amu_wph, double nHTot) { return amu_wph * nHTot; }

// hTau1 = np.interp(1.0, tau, height) (:104, :136) found while tau and height are made, depth after depth
struct Tau1 { double h; int found; };

LSXBG_HD void tau1_first(Tau1& q, double tau0, double h0)
{
    q.found = 1.0 < tau0;          // below the first point: numpy returns fp[0]
    q.h = h0;
}

LSXBG_HD void tau1_next(Tau1& q, double tau_p, double h_p, double tau, double h)
{
    if (q.found || !(tau_p <= 1.0 && 1.0 < tau)) return;
    q.found = 1;
    if (tau_p == 1.0) { q.h = h_p; return; }
    const double slope = (h - h_p) / (tau - tau_p);
    q.h = slope * (1.0 - tau_p) + h_p;
}

// 1 >= tau[-1]: fp[-1]
LSXBG_HD double tau1_last(const Tau1& q, double h_last) { return q.found ? q.h : h_last; }

struct Run {                       // a column at the depth just made
    double height, cmass, tau, rho, chi;
    Tau1 t1;
};

// depth 0.  ds0, ds1: the depth scale at depths 0 and 1 (ds1 is read for the geometric scale only, like t0, nH0, ne0, wph, gravity)
template <int SCALE>
LSXBG_HD void start(Run& R, double ds0, double ds1, double rho0, double chi0, double t0, double nH0, double ne0, double wph, double gravity)
{
    R.rho = rho0;
    R.chi = chi0;
    if (SCALE == COLUMN_MASS) {            // :98-99
        R.cmass = ds0;
        R.height = 0.0;
        R.tau = chi0 / rho0 * ds0;
    } else if (SCALE == GEOMETRIC) {       // :115-118
        R.height = ds0;
        R.cmass = (nH0 * wph + ne0) * (KBOLTZMANN * t0 / gravity);
        R.tau = 0.5 * chi0 * (ds0 - ds1);
        if (R.tau > 1.0) R.tau = 0.0;
    } else {                               // :131
        R.tau = ds0;
        R.height = 0.0;
        R.cmass = (ds0 / chi0) * rho0;
    }
    tau1_first(R.t1, R.tau, R.height);
}

// depth k >= 1 from depth k - 1
template <int SCALE>
LSXBG_HD void step(Run& R, double ds, double rho, double chi)
{
    const double h_p = R.height, tau_p = R.tau;
    if (SCALE == COLUMN_MASS) {            // :101-102
        R.height = h_p - 2.0 * (ds - R.cmass) / (R.rho + rho);
        R.tau = tau_p + 0.5 * (R.chi + chi) * (h_p - R.height);
        R.cmass = ds;
    } else if (SCALE == GEOMETRIC) {       // :121-122
        R.cmass = R.cmass + 0.5 * (R.rho + rho) * (h_p - ds);
        R.tau = tau_p + 0.5 * (R.chi + chi) * (h_p - ds);
        R.height = ds;
    } else {                               // :133-134 (cmass integrates chi_c, as the reference has it)
        R.height = h_p - 2.0 * (ds - tau_p) / (R.chi + chi);
        R.cmass = R.cmass + 0.5 * (R.chi + chi) * (h_p - R.height);
        R.tau = ds;
    }
    R.rho = rho;
    R.chi = chi;
    tau1_next(R.t1, tau_p, h_p, R.tau, R.height);
}

} // namespace lsxsc
