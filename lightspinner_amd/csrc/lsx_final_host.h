// lsx_final_host.h -- host side of what the final passes share: the argument rules of their entry points, the
// column-independent tables of the context's own grid and the fill of the kernel parameters that name them (lsx_rays.hip,
// lsx_rates.hip, lsx_losses.hip, lsx_depth.hip, lsx_stokes.hip, lsx_stokes_response.hip; lsx_spectrum.hip takes the argument rules and
// final_fill_angles only: its tables depend on the call's wavelengths).  `who` is the entry point's name in the messages.  The buffers
// of the passes (GrowBuf), the description of a Stokes call and what the Stokes units share: lsx_ctx.h; the columns of a pass: lsx_plan.h.
#pragma once
#include <algorithm>
#include <vector>

#include "lsx_ctx.h"
#include "lsx_final_dev.h"

namespace lsxd {

// ---- the argument rules the entry points share; each entry calls them in the order it always tested them ----
// the angles of a call
inline int final_check_angles(const char* who, int32_t nmu, const double* mu)
{
    if (nmu < 1) return fail(LSX_EINVAL, "%s: nmu = %d, need at least one angle", who, (int)nmu);
    for (int m = 0; m < nmu; ++m)
        if (!(mu[m] > 0.0 && mu[m] <= 1.0)) return fail(LSX_EINVAL, "%s: mu[%d] = %g is outside (0, 1]", who, m, mu[m]);
    return LSX_OK;
}

inline int final_check_range(const lsx_ctx* c, const char* who, int32_t col0, int32_t ncol)
{
    if (col0 < 0 || ncol < 1 || (int64_t)col0 + ncol > c->ncol)
        return fail(LSX_EINVAL, "%s: columns [%d, %d) are outside the context's %d", who, (int)col0, (int)col0 + (int)ncol, c->ncol);
    return LSX_OK;
}

// a call's window [la0, la0 + nla) of the merged wavelength grid
inline int final_check_window(const lsx_ctx* c, const char* who, int32_t la0, int32_t nla)
{
    if (nla < 1) return fail(LSX_EINVAL, "%s: nla = %d, need at least one wavelength", who, (int)nla);
    if (la0 < 0 || (int64_t)la0 + nla > c->Nspect)
        return fail(LSX_EINVAL, "%s: wavelengths [%d, %d) are outside the grid's %d", who, (int)la0, (int)la0 + (int)nla, c->Nspect);
    return LSX_OK;
}

inline int final_check_depths(const lsx_ctx* c, const char* who)
{
    if (c->Nspace < 3) return fail(LSX_EUNSUPPORTED, "%s: needs Nspace >= 3", who);
    return LSX_OK;
}

// what a pass asks of the state of columns [col0, col0 + ncol) (a checked range).  A pass on the context's own rays and wavelengths
// (rates, losses) only needs line profiles; one at another angle (rays, depth) or at another wavelength (spectrum) must also be able
// to form them there
enum FinalAt { FINAL_OWN_RAYS, FINAL_OTHER_ANGLE, FINAL_OTHER_WAVELENGTH };
inline int final_check_columns(const lsx_ctx* c, const char* who, int32_t col0, int32_t ncol, FinalAt at)
{
    const bool wl = at == FINAL_OTHER_WAVELENGTH;
    for (int q = col0; q < col0 + ncol; ++q) {
        if (at != FINAL_OWN_RAYS && !c->bnd_kind.empty() && c->bnd_kind[2 * (size_t)q] == LSX_BOUNDARY_GIVEN)
            return fail(LSX_EUNSUPPORTED, "%s: column %d has a GIVEN lower boundary (lsx_hip_set_boundary): its intensity was handed "
                                          "over on the context's own rays and wavelengths and is not known at another %s", who, q,
                        wl ? "angle or wavelength" : "angle");
        if (!c->phi_set[q])
            return fail(LSX_EINVAL, "%s: column %d has no line profiles (lsx_set_columns with phi == NULL must be "
                                    "followed by lsx_set_line_profiles)", who, q);
        if (at != FINAL_OWN_RAYS && c->Nlines && (wl || !c->phi_compact) && (c->prof_kind.empty() || !c->prof_kind[q]))
            return fail(LSX_EUNSUPPORTED, "%s: the %sline profiles of column %d were handed over as arrays "
                                          "(lsx_set_columns): the library cannot know them at another %s.  Build them with "
                                          "lsx_set_line_profiles or lsx_set_atmosphere", who, wl ? "" : "ray-dependent ", q,
                        wl ? "wavelength" : "angle");
    }
    return LSX_OK;
}

// column-independent tables of the context's grid, made by the first final pass that needs them: per wavelength its active
// transitions in table order (FinalEnt) and its place in the tile-major streams; per transition its row of nsr
inline int final_tables(lsx_ctx* c, const char* who)
{
    if (c->d_final_ptr) return LSX_OK;
    const int Nspect = c->Nspect;
    std::vector<int32_t> la_tile(2 * (size_t)Nspect, 0), ptr(Nspect + 1, 0);
    std::vector<int> tile_of(Nspect, -1);
    for (size_t t = 0; t < c->tiles.size(); ++t)
        for (int q = 0; q < c->tiles[t].nla; ++q) {
            const int la = c->tiles[t].la0 + q;
            tile_of[la] = (int)t;
            la_tile[2 * la] = (int32_t)t;
            la_tile[2 * la + 1] = q;
        }
    std::vector<FinalEnt> ents;
    for (int la = 0; la < Nspect; ++la) {
        if (tile_of[la] < 0) return fail(LSX_EDEVICE, "%s: wavelength %d belongs to no tile", who, la);
        const DevTile& tl = c->tiles[tile_of[la]];
        for (int t = 0; t < c->Ntrans; ++t) {
            if (!c->active[(size_t)t * Nspect + la]) continue;
            const DevTrans& h = c->htrans[t];
            const int lt = la - h.Nblue;
            if (lt < 0 || lt >= h.Nlam) return fail(LSX_EDEVICE, "%s: transition %d is active outside its range at wavelength %d", who, t, la);
            FinalEnt e{};
            e.is_line = h.is_line; e.li = h.li; e.lj = h.lj; e.row = c->trans_row[t]; e.atom = h.atom;
            if (h.is_line) {
                const DevSlot* sl = nullptr;
                for (int u = 0; u < tl.nL; ++u)
                    if (c->slots[tl.slot0 + u].trans == t) sl = &c->slots[tl.slot0 + u];
                if (!sl || !(sl->flags & SLOT_LINE) || la < sl->first || la >= sl->first + sl->len)
                    return fail(LSX_EDEVICE, "%s: line %d has no profile block at wavelength %d", who, t, la);
                e.phi_base = sl->base; e.phi_len = sl->len; e.phi_l = la - sl->first;
                e.cell = h.phi_off + lt;
                e.a = h.cB; e.g = h.gij; e.Uc = h.AB * (h.gij * h.cB); e.lambda0 = h.lambda0;
            } else {
                e.a = c->alpha[h.wl_off + lt];
            }
            ents.push_back(e);
        }
        ptr[la + 1] = (int32_t)ents.size();
    }
    if (ents.empty()) ents.push_back(FinalEnt{});
    std::vector<int32_t> rows(c->trans_row.begin(), c->trans_row.end());
    rows.resize(std::max(1, c->Ntrans), 0);
    int rc = upload(&c->d_final_tile, la_tile, c->stream);
    if (!rc) rc = upload(&c->d_final_row, rows, c->stream);
    if (!rc) rc = upload(&c->d_final_ent, ents, c->stream);
    if (!rc) rc = upload(&c->d_final_ptr, ptr, c->stream);       // (last: its presence marks the set complete)
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));                      // the host vectors go out of scope
    return LSX_OK;
}

// ---- the kernel parameters the passes share: the host side of final_column<P> and final_angles<P> (lsx_final_dev.h), which read
// these fields by name from every unit's parameter struct.  What is a unit's own stays in the unit ----
// what final_column and the tables need: dimensions, strides, the grid, the tables (final_tables has run), the state of the columns
template <typename P>
void final_fill(P& p, const lsx_ctx* c)
{
    p.Ns = c->Nspace; p.Nspect = c->Nspect; p.NLtot = c->NLtot; p.Ncont = c->Ncont; p.L = c->L; p.Nrays = c->Nrays;
    p.phi_compact = c->phi_compact; p.sca_per_lambda = c->sca_per_lambda; p.phi_G = c->phi_group;
    p.til_col = (int64_t)c->til_col; p.phi_col = (int64_t)c->phi_col; p.sca_col = (int64_t)c->sca_col;
    p.wavelength = c->d_wavelength; p.u_la = c->d_u_la; p.exp2_tab = c->d_exp2_tab;
    p.la_ptr = c->d_final_ptr; p.ents = c->d_final_ent; p.la_tile = c->d_final_tile;
    p.height = c->d_height; p.temperature = c->d_temperature; p.n = c->d_n; p.nsr = c->d_nsr;
    p.bgchi_T = c->d_bgchi; p.bgeta_T = c->d_bgeta; p.J_T = c->d_J[c->jcur];      // what lsx_get(LSX_J) returns at this moment
    p.E_T = c->d_E; p.sca = c->d_sca; p.phi_T = c->d_phi;
    p.bnd = c->d_bnd;
}

// what final_angles needs: the kept broadening arrays, from which a profile is formed at another angle or wavelength
template <typename P>
void final_fill_angles(P& p, const lsx_ctx* c)
{
    p.Natoms = c->Natoms; p.NlinesA = std::max(1, c->Nlines);
    p.voigt_W = c->d_voigt_w;
    p.aDamp = c->d_aDamp; p.vBroad = c->d_vBroad; p.vlos = c->d_vlos; p.prof_kind = c->d_prof_kind;
}

} // namespace lsxd
