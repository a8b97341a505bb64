// lsx_solve_flag.h -- what a solve kernel (lsx_hip.hip: k_stat_equil, k_stat_equil_reg; lsx_timedep.hip: k_time_dep,
// k_time_dep_reg) leaves behind for lsx_sync / lsx_last_error: the singular flag and the per-column monitor.  Device code, and
// the one constant the host's decoder shares with it.
#pragma once
#include <hip/hip_runtime.h>

namespace lsxd {

// singular system at (column, atom, depth): the flag keeps the FIRST one in that order, the one the reference raises on (it walks
// the atoms outside the depths, rh_method.py:720-739, and the columns one after the other) -- one order-independent 64-bit
// atomicMax of (2^48 - key), key = (column << 8 | atom) Nspace + depth, 0 = none -- for lsx_last_error (cf. LinAlgError)
constexpr unsigned long long kSingBase = 1ull << 48;
__device__ __forceinline__ void flag_singular(unsigned long long* flag, int col, int atom, int k, int Ns)
{
    atomicMax(flag, kSingBase - ((((unsigned long long)col << 8) | (unsigned)atom) * (unsigned long long)Ns + (unsigned)k));
}

// dPcol[col] = max(dPcol[col], v) for the lanes of a wave that are here (v: a non-negative, non-NaN double as its bit pattern,
// which orders like the value; 0: nothing to record), with ONE atomic per run of lanes that hold the same column, not one per
// lane: consecutive lanes hold consecutive depths, so a wave is one or two runs at 82 depths.  The per-lane atomics of 82 000
// points were 18 of the statistical equilibrium's 30 us on 1000 columns (profiles/serial_tail/README.md).  A maximum does not
// depend on the order it is taken in: the same bits.  The lanes of a run reduce by shuffles from higher lanes (a lane takes
// lane + d's value if that lane is here and holds the same column: after d = 1, 2, ... 32 the first lane of every stretch without
// a gap holds the stretch's maximum or more of its column's); every lane that starts a stretch -- lane 0, a lane behind one
// that has left (past the end, a frozen column, a refused system), the first lane of a column -- issues the atomic.
__device__ __forceinline__ void column_max(double* dPcol, int col, unsigned long long v)
{
    const int lane = __lane_id();
    const unsigned long long here = __ballot(1);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int oc = __shfl_down(col, d);
        const unsigned long long ov = __shfl_down(v, d);
        if (lane + d < 64 && ((here >> (lane + d)) & 1) && oc == col && ov > v) v = ov;
    }
    const int pc = __shfl_up(col, 1);
    const bool first = lane == 0 || !((here >> (lane - 1)) & 1) || pc != col;
    if (first && v) atomicMax(reinterpret_cast<unsigned long long*>(&dPcol[col]), v);
}

// the end of every solve kernel: a singular system is flagged; otherwise maxRelChange = max(maxRelChange, change.max()) with
// Python's builtin max (rh_method.py:741) -- a NaN never replaces the running maximum, so a depth whose change is NaN drops out.
// Every lane that solved a point calls it, whatever the outcome (column_max needs the wave's lanes together).
__device__ __forceinline__ void record_solve(bool solved, double change, unsigned long long* singular, double* dPcol, int col,
                                             int atom, int k, int Ns)
{
    if (!solved) flag_singular(singular, col, atom, k, Ns);
    column_max(dPcol, col, solved && change == change ? static_cast<unsigned long long>(__double_as_longlong(fabs(change))) : 0ull);
}

} // namespace lsxd
