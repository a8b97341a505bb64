// lsx_ctx.h -- the context object behind the C ABI and the helpers the host-side translation units share
// (lsx_hip.hip: runtime + small kernels, lsx_setup.hip: set-up chain).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../include/lsx.h"
#include "lsx_dev.h"
#include "lsx_plan.h"

namespace lsxd {
extern thread_local std::string g_err;
int fail(int code, const char* fmt, ...);    // records the message lsx_last_error returns; -> code
struct FinalEnt;                             // an entry of the final passes' tables (lsx_final_dev.h)

// What an internal caller of the Stokes pass or of its response hands over to keep a pass's result on the device (lsx_fit.hip): pass()
// is called in the place of the pass's copy to the host, behind the pass's launches, with the pass's first column counted from the
// call's col0, its number of columns and the pass's device array.  It queues its work on the context's stream; the caller of pass()
// waits for the stream before the array is used again.
struct PassSink {
    virtual int pass(size_t b0, size_t nb, const double* d_result) = 0;
protected:
    ~PassSink() = default;
};
// What a Stokes pass is asked for, as lsx_hip_stokes_rays takes it (include/lsx_hip_stokes.h): angles, columns, window of the merged
// grid, the field of the call's columns ([ncol][Nspace] each) and the Zeeman patterns of the lines.  The entries build it from their
// arguments, in this order; lsx_fit.hip builds one per group of columns.  vlos (include/lsx_hip_stokes_velocity.h): null, or the
// line-of-sight velocity of the call's columns [ncol][Nspace], which stands in the place of the context's in this pass alone
struct StokesCall {
    int32_t nmu;
    const double* mu;
    int32_t col0, ncol, la0, nla;
    const double *B, *gammaB, *chiB;
    const int32_t *ncomp, *alpha;
    const double *strength, *shift;
    const double* vlos = nullptr;
    int nfield() const { return vlos ? 4 : 3; }        // the arrays of [ncol][Nspace] a pass uploads
};
// the bodies of lsx_hip_stokes_rays (lsx_stokes.hip) and lsx_hip_response_stokes (lsx_stokes_response.hip); `who` heads the messages.
// amplitude: [3], or [4] where the call has a velocity (bit 8 of params, the response to vlos, is accepted only then)
int stokes_rays_run(lsx_ctx* c, const char* who, const StokesCall& s, double* out, size_t nbytes, PassSink* sink);
int response_stokes_check(lsx_ctx* c, const char* who, const StokesCall& s, uint32_t params, const double* amplitude, int32_t nk,
                          const int32_t* ks);
int response_stokes_run(lsx_ctx* c, const char* who, const StokesCall& s, uint32_t params, const double* amplitude, int32_t nk,
                        const int32_t* ks, double* rf, size_t rf_bytes, const size_t* stokes_bytes, PassSink* sink);
// What the two passes share on the host (lsx_stokes.hip).  The argument rules every Stokes call answers to, in the order
// lsx_hip_stokes_rays always tested them, in two halves because that entry tests its byte count between them: what the call says
// about itself (null arguments, ncomp, angles, columns, window) ...
int stokes_check_call(const lsx_ctx* c, const char* who, const StokesCall& s);
// ... and what it asks of the field, the patterns and the state of its columns
int stokes_check_state(const lsx_ctx* c, const char* who, const StokesCall& s);
// the patterns of the lines that are active somewhere in the window, packed for the device (lsx_stokes_prep.h, pack_patterns)
int stokes_patterns(const lsx_ctx* c, const char* who, const StokesCall& s, std::vector<int32_t>& pat_line, std::vector<double>& pat_tab);
// the field of a pass: columns [b0, b0 + nb) of the call's three arrays (and of its velocity, if it has one, as the fourth) to
// d_field, nb * Nspace doubles each, that far apart
int stokes_upload_field(lsx_ctx* c, const StokesCall& s, size_t b0, size_t nb, double* d_field);

// The device buffers that grow with the calls: the work arrays of the passes under a cap, and the tables of a call.  One per purpose;
// they never share storage (the fit holds its own while the Stokes and the response pass run inside it, the response entry runs the
// Stokes pass behind its own).  lsx_destroy releases all of lsx_ctx::buf: a new buffer is a new name here and nothing else
enum FinalBuf {
    // the work arrays of lsx_hip_radiative_rates (lsx_rates.hip), allocated at first use, under the cap (0: include/lsx_hip_rates.h's)
    BUF_RATES_WORK,
    // ... of lsx_hip_radiative_losses (lsx_losses.hip; cap 0: the default of include/lsx_hip_losses.h)
    BUF_LOSSES_WORK,
    // ... of lsx_hip_depth_rays (lsx_depth.hip; cap 0: the default of include/lsx_hip_depth.h)
    BUF_DEPTH_WORK,
    // ... and of lsx_hip_spectrum (lsx_spectrum.hip): the tables of a call (they depend on the call's wavelengths: rebuilt per call,
    // the buffer grows as needed) and the arrays of a pass (allocated at first use; cap 0: the default of include/lsx_hip_spectrum.h)
    BUF_SPEC_TAB, BUF_SPEC_WORK,
    // ... and of lsx_hip_stokes_rays (lsx_stokes.hip): the Zeeman pattern tables of a call (rebuilt per call, the buffer grows as
    // needed) and the angles, the field and the result of a pass (allocated at first use; cap 0: include/lsx_hip_stokes.h's)
    BUF_STOKES_TAB, BUF_STOKES_WORK,
    // ... and of lsx_hip_response_stokes (lsx_stokes_response.hip): pattern tables and requested depths of a call, and the arrays of
    // a pass (angles, field, nodes, kept states, the two results; cap 0: the default of include/lsx_hip_stokes_response.h)
    BUF_STRESP_TAB, BUF_STRESP_WORK,
    // ... and of the field fit (lsx_fit.hip): basis, observation, weights, the kept Stokes vectors, the Jacobian and the sums of a
    // group of columns (cap 0: the default of include/lsx_hip_fit.h)
    BUF_FIT_WORK,
    BUF_COUNT
};
struct GrowBuf {
    char* p = nullptr;
    size_t bytes = 0;
    size_t cap = 0;             // what the buffer's unit keeps its passes under, in bytes; 0: the default of the unit's header
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
    // at least nbytes: nothing if they are there; else behind the context's stream the old array goes and a new one is made (a failed
    // allocation leaves the buffer empty)
    int reserve(lsx_ctx* c, size_t nbytes);
    // the whole of a unit's _work_cap entry `who`: the array goes, the next call allocates under the new cap
    static int set_cap(lsx_ctx* c, FinalBuf b, const char* who, size_t nbytes);
    void release();             // lsx_destroy
};
} // namespace lsxd

#define HIPCHK(expr)                                                                                    \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return lsxd::fail(LSX_EDEVICE, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

struct SweepClass : lsxd::PlanClass {   // a plan class + what the runtime keeps for it: its own stream, events, device tile lists
    long launches = 0;         // how often this class's kernel has been launched (introspection for the tests)
    hipEvent_t tdone = nullptr; // timed runs: end of this class's launch
    int* d_fast_tiles = nullptr;
    int *d_fast_cols[LSX_FGC_LISTS] = {}, *d_fast_rest = nullptr;
    int* d_tiles = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
};

// launches of the kernels behind the sweep since the context was made (introspection for the tests: lsx_hip_epilogue_info,
// tests/test_epilogue_instances.py); kept beside SweepClass::launches and counted where those are
struct EpilogueLaunches {
    long rows[LSX_FAST_ROWS_NINST] = {};   // k_fast_gamma<LP, NT, SEG>, by lsx_fast_rows_index
    long cols[LSX_FGC_LISTS] = {};         // k_fast_gamma_cols / k_fast_gamma_cols_big, per tile list
    long prepass[2] = {};                  // k_fast_prepass<SEG>
    long finish[3] = {};                   // k_gamma_finish_small, k_gamma_finish_levels, k_gamma_finish
    void add(const EpilogueLaunches& a, const EpilogueLaunches& b)      // += a - b
    {
        for (int i = 0; i < LSX_FAST_ROWS_NINST; ++i) rows[i] += a.rows[i] - b.rows[i];
        for (int i = 0; i < LSX_FGC_LISTS; ++i) cols[i] += a.cols[i] - b.cols[i];
        for (int i = 0; i < 2; ++i) prepass[i] += a.prepass[i] - b.prepass[i];
        for (int i = 0; i < 3; ++i) finish[i] += a.finish[i] - b.finish[i];
    }
};

struct FsGraphKey {            // what a captured formal solution's kernel arguments depend on beyond the context's fixed state
    int jcur; const void* results; int clear_dp, solver, policy, policy_columns; const void* colmask;
    bool operator==(const FsGraphKey& o) const
    {
        return jcur == o.jcur && results == o.results && clear_dp == o.clear_dp && solver == o.solver && policy == o.policy &&
               policy_columns == o.policy_columns && colmask == o.colmask;
    }
};

struct lsx_ctx : lsxd::LsxPlan {        // the plan (lsx_plan.h: dimensions, tables, tile schedule, strides, launch shapes) + device state
    int device = 0;
    lsxd::CtxOptions options;       // what lsx_create_with_options ended up with (environment defaults + explicit list)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int ncol = 0;
    DevSlot* d_slots = nullptr;
    std::vector<SweepClass> classes;     // plan_classes, in launch order
    hipEvent_t ev_fork = nullptr;
    double ms_sweep = 0.0, ms_finish = 0.0;
    double ms_epi_tail = 0.0;   // lsx_time_formal_sol: join - end of the last class's sweep (exposed fast-continuum epilogue)
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    // device: column independent
    double *d_wavelength = nullptr, *d_zmu = nullptr, *d_wmuh = nullptr, *d_wl = nullptr, *d_alpha = nullptr,
           *d_u_la = nullptr, *d_fgtab = nullptr;
    int* d_level_atom = nullptr;
    uint8_t* d_active = nullptr;
    DevTrans* d_trans = nullptr;
    DevTile* d_tiles = nullptr;
    int *d_tile_slots = nullptr, *d_Nlevel = nullptr, *d_lev2_off = nullptr, *d_fin_ptr = nullptr, *d_fin_idx = nullptr, *d_atom_ptr = nullptr, *d_atom_slots = nullptr;
    bool dp_zeroed = false;          // the Gamma epilogue has zeroed dPcol / the singular flag for the next stat_equil
    bool opt_finish_big = false;     // LSX_FINISH_BIG=1: the many-column Gamma epilogue also for small batches (tests)
    bool opt_graph = false;          // LSX_GRAPH=1: a formal solution's launches as a captured HIP graph (enqueue_fs; measurement)
    std::vector<std::pair<FsGraphKey, hipGraphExec_t>> fs_graphs;
    std::vector<EpilogueLaunches> fs_graph_epi;   // ... and the epilogue launches each of them replays
    bool opt_fused_epilogue = false; // LSX_FUSED_EPILOGUE=1: the fused launch also runs its fast tiles' Gamma epilogue (measured: slower, see enqueue_fs)
    int opt_abl_fast = 0;            // LSX_ABL_FUSED_FAST: timing ablations of the fused launch's fast-continuum work
    bool opt_no_fused_fast = false;  // LSX_NO_FUSED_FAST=1: small batches launch the fast-continuum kernels around the fused sweep (tests)
    // device: per column
    double *d_height = nullptr, *d_temperature = nullptr, *d_nStar = nullptr, *d_nTotal = nullptr, *d_n = nullptr,
           *d_C = nullptr, *d_Gamma = nullptr, *d_wphi = nullptr, *d_bgchi = nullptr, *d_bgeta = nullptr, *d_bgce = nullptr, *d_bgxce = nullptr,
           *d_sca = nullptr, *d_phi = nullptr, *d_E = nullptr, *d_corr = nullptr, *d_Psi3 = nullptr, *d_J[2] = {nullptr, nullptr}, *d_I = nullptr,
           *d_Gpart = nullptr, *d_dJpart = nullptr, *d_dJcol = nullptr, *d_dPcol = nullptr, *d_res = nullptr;
    unsigned long long* d_singular = nullptr;
    std::vector<uint8_t> phi_set;    // per column: line profiles have been handed over or built
    std::vector<uint8_t> cols_set;   // per column: lsx_set_columns has run (geometry and temperature are there; lsx_hip_background)
    size_t n_phi_set = 0;
    int solver = 0;               // LSX_SOLVER_* (lsx_set_formal_solver)
    int sweep_policy = LSX_SWEEP_AUTO;   // lsx_set_sweep_policy: which wavefront mapping the formal solution runs ...
    int policy_columns = 0;              // ... and, under AUTO, the column count that decides (0: this context's own)
    bool opt_se_lds = false, opt_trace_classes = false, opt_serial = false;   // LSX_SE_LDS / LSX_TRACE_CLASSES / LSX_SERIAL, read once in lsx_create
    long fused_launches = 0;
    EpilogueLaunches epi_launches;
    uint8_t* d_colmask = nullptr; // per-column activity, nullptr = all active
    std::vector<uint8_t> colmask_host;   // host copy of the same (empty: all active)
    double *d_bgxchi = nullptr, *d_bgxeta = nullptr, *d_Psi2 = nullptr; // fast-continuum side arrays
    int* d_fast_tiles = nullptr;
    int *d_fast_cols[LSX_FGC_LISTS] = {}, *d_fast_rest = nullptr;
    int *d_cont_li = nullptr, *d_cont_lj = nullptr;
    double* d_exp2_tab = nullptr;
    double* d_voigt_w = nullptr;
    double *d_muz = nullptr, *d_wmu = nullptr;
    double* d_nsr = nullptr;     // [col][Ncont][k] nStar_i / nStar_j of the continua
    double* d_optab = nullptr;   // ray-serial sweep: per-depth operands per (column group, transition) + geometry (lsx_plan.h), made on first use
    int* d_trans_row = nullptr;  // per transition: row of wphi / nsr
    bool optab_fresh = false;    // d_optab was built from the current n, wphi, nStar ratios, heights and sigma
    double* d_debug = nullptr;   // 64 x 16 x 8 B, diagnostic builds of the sweep kernel write stamps here
    int jcur = 0; // d_J[jcur] holds the current J (Jdag of the next call)
    // set-up chain (lsx_setup.hip): atomic data tables and what lsx_set_atmosphere derives per column
    char *d_sa_atoms = nullptr, *d_sa_lines = nullptr, *d_sa_colls = nullptr;
    double *d_sa_spl = nullptr, *d_sa_levE = nullptr, *d_sa_levg = nullptr, *d_sa_levnD = nullptr;
    int32_t* d_sa_levdZ = nullptr;
    bool have_atomic_data = false;
    double *d_vBroad = nullptr, *d_aDamp = nullptr;     // [col][Natoms][k], [col][Nlines][k]
    // what the line profiles of a column were built from is KEPT (vBroad and aDamp above, and the line-of-sight velocity), whichever
    // entry built them (lsx_set_line_profiles, lsx_set_atmosphere): the final pass at other angles re-evaluates ray-dependent
    // profiles from it (lsx_rays.hip)
    double* d_vlos = nullptr;            // [col][k], zero where none was given
    uint8_t* d_prof_kind = nullptr;      // per column: 0 profiles handed over as arrays (or none yet), 1 built without, 2 with a velocity
    std::vector<uint8_t> prof_kind;      // host copy of the same
    bool atm_arrays = false;             // lsx_set_atmosphere has run: LSX_VBROAD / LSX_ADAMP can be read back
    // column-independent tables of the final passes over the context's own grid, made on first use (final_tables, lsx_final_host.h)
    int32_t *d_final_ptr = nullptr, *d_final_tile = nullptr, *d_final_row = nullptr;
    lsxd::FinalEnt* d_final_ent = nullptr;
    // the work arrays and the per-call tables of the final passes, by lsxd::FinalBuf (above: what each holds)
    lsxd::GrowBuf buf[lsxd::BUF_COUNT];
    // the weights of a call of lsx_hip_radiative_losses (losses_wnu: the trapezoid rule in frequency over the merged grid, the default)
    double* d_losses_wnu = nullptr;
    std::vector<double> losses_wnu;
    // Ng acceleration of the populations (lsx_ng.hip, include/lsx_hip_ng.h): off (order 0) unless lsx_hip_ng_configure turns it on
    int ng_order = 0, ng_delay = 0;
    double* d_ng_hist = nullptr;         // [col][order + 2][NLtot][k]: the stored populations, slot = the column's counter
    int32_t* d_ng_state = nullptr;       // [3][ncol]: counter, steps taken, steps rejected
    double* d_ng_coef = nullptr;         // [col][Natoms][2]: the coefficients of the last step taken
    int* d_ng_off = nullptr;             // [Natoms + 1]: where each atom's levels x depths start in a column's populations
    // time-dependent populations (lsx_timedep.hip, include/lsx_hip_timedep.h): allocated by the first lsx_hip_time_dep_start
    double* d_td_n_prev = nullptr;       // [col][NLtot][k]: the populations at the start of the column's time step
    double* d_td_dt = nullptr;           // [col]: the time step, 0 = no step started
    std::vector<double> td_dt;           // host copy of d_td_dt
    // the radiation boundary (lsx_boundary.hip, include/lsx_hip_boundary.h): nothing until lsx_hip_set_boundary is first called
    int32_t* d_bnd = nullptr;            // the boundary store (lsx_dev.h): what the kernels test: null = the hard-wired pair, code as it was
    bool bnd_values = false;             // ... holds the start values too (re-allocated with them at the first GIVEN)
    std::vector<int32_t> bnd_kind;       // host copy of the kinds in the store, [col][2] = (lower, upper) (empty: never set)
    // staging
    double* d_stage = nullptr;
    size_t stage_doubles = 0;
    double* h_pinned = nullptr; // host mirror of d_res
    double* h_n = nullptr;      // pinned host mirror of the populations (lsx_sync_begin_populations), made on first use
    bool h_n_pending = false, h_n_valid = false;      // a read-back of n is in flight / has been collected by lsx_sync_end
    double last_dJ = 0.0, last_dP = 0.0;
    bool fs_pending = false, se_pending = false;
    hipEvent_t evA = nullptr, evB = nullptr;
    // pipelined MALI loop (include/lsx.h: lsx_sync_begin / lsx_formal_sol_gamma_speculative / lsx_discard_formal_sol): the second set
    // of the buffers a formal solution overwrites (J already is a pair), and the read-back in flight
    double *d_I_alt = nullptr, *d_Gamma_alt = nullptr, *d_res_alt = nullptr;
    bool spec_valid = false;         // the last formal solution was speculative and nothing has built on it: it can be discarded
    bool spec_dp_zeroed = false;     // dp_zeroed as it was before that call
    bool spec_fs_pending = false;    // fs_pending likewise
    double spec_last_dJ = 0.0;       // last_dJ likewise
    bool mon_spec = false;           // the read-back in flight was begun while a speculative call could still be discarded
    bool mon_outstanding = false, mon_fs = false, mon_se = false;
    hipEvent_t ev_mon = nullptr;
};

namespace lsxd {

// the column count the bit-relevant kernel choices are made for (include/lsx.h, lsx_set_sweep_policy)
inline int policy_ncol(const lsx_ctx* c) { return c->policy_columns > 0 ? c->policy_columns : c->ncol; }
// the ray-serial mapping (classes that have an instance of it for the context's rule) or one ray per lane
inline bool use_ray_serial(const lsx_ctx* c)
{
    if (!c->rs_ok || c->sweep_policy == LSX_SWEEP_RAY_PER_LANE) return false;
    return c->sweep_policy == LSX_SWEEP_RAY_SERIAL || policy_ncol(c) >= c->rs_min_columns;
}
// one launch per tile class on forked streams (else: one fused launch on the context's stream).  For the linear rule the two
// give the same bits per mapping, so the context's OWN size decides unless the ray-serial kernels run (they exist per class
// only); the parabolic rule's compile-time classes and its generic instance differ in the last bits: the policy count decides.
inline bool per_class_launches(const lsx_ctx* c)
{
    if (c->solver == LSX_SOLVER_PARABOLIC) return policy_ncol(c) >= 32 || use_ray_serial(c);
    return c->ncol >= 32 || use_ray_serial(c);
}

template <typename T>
int dmalloc(T** p, size_t count)
{
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
    if (e != hipSuccess) return fail(LSX_EDEVICE, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
    return LSX_OK;
}

inline int GrowBuf::reserve(lsx_ctx* c, size_t nbytes)
{
    if (bytes >= nbytes) return LSX_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (p) HIPCHK(hipFree(p));
    p = nullptr;
    bytes = 0;
    const int rc = dmalloc(&p, nbytes);
    if (rc) return rc;
    bytes = nbytes;
    return LSX_OK;
}

inline int GrowBuf::set_cap(lsx_ctx* c, FinalBuf b, const char* who, size_t nbytes)
{
    if (!c) return fail(LSX_EINVAL, "%s: null context", who);
    GrowBuf& w = c->buf[b];
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (w.p) HIPCHK(hipFree(w.p));
    w.p = nullptr;
    w.bytes = 0;
    w.cap = nbytes;
    return LSX_OK;
}

inline void GrowBuf::release()
{
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
}

template <typename T>
int upload(T** dptr, const std::vector<T>& v, hipStream_t st)
{
    int rc = dmalloc(dptr, v.size());
    if (rc) return rc;
    if (!v.empty()) HIPCHK(hipMemcpyAsync(*dptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return LSX_OK;
}

int ensure_stage(lsx_ctx* c, size_t doubles);    // grow the context's staging buffer
int rebuild_derived(lsx_ctx* c, size_t col0, size_t ncol);     // continuum g_ij tables + nStar ratios from (nStar, T)
// the background of columns [col0, col0 + ncol) from DEVICE arrays in the layout lsx_set_columns takes from the host (chi, eta:
// [ncol][Nspect][Nspace]; sca: [ncol][Nspace], or like chi where sca_per_lambda): lsx_set_columns' own steps behind its uploads
int background_from_device(lsx_ctx* c, size_t col0, size_t ncol, const double* d_chi, const double* d_eta, const double* d_sca);
int profiles_from_device(lsx_ctx* c, size_t col0, size_t ncol, const double* dA, const double* dV, const double* dL);
void profiles_handed_over(lsx_ctx* c, size_t col0, size_t ncol);    // these columns' profiles no longer come from kept inputs
void mark_profiles_set(lsx_ctx* c, size_t col0, size_t ncol);
// One solve of every atom's populations behind the last formal solution, on the context's stream (lsx_hip.hip): the statistical
// equilibrium or the time-dependent step, which differ in the kernels that launch(c, atom, grid, block, lds) starts -- lds bytes
// of LDS for the in-memory kernel, 0 for the register instance of the atom's level count.  Refuses (`what` names the caller)
// before anything is launched; zeroes the monitors where the Gamma epilogue has not, enqueues Ng and marks the solve pending.
int enqueue_solves(lsx_ctx* c, const char* what, void (*launch)(lsx_ctx*, int, dim3, dim3, size_t));
// Ng acceleration (lsx_ng.hip); all three do nothing while it is off
int ng_enqueue(lsx_ctx* c);                              // the step behind a statistical equilibrium, on the context's stream
int ng_reset(lsx_ctx* c, size_t col0, size_t ncol);      // these columns' populations have been replaced: their history is discarded
void ng_free(lsx_ctx* c);
void td_free(lsx_ctx* c);                                // the state of the time-dependent step (lsx_timedep.hip)
void boundary_free(lsx_ctx* c);                          // the radiation boundary (lsx_boundary.hip)

} // namespace lsxd
