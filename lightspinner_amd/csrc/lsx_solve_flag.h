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

__device__ __forceinline__ void atomic_max_nonneg(double* addr, double v)
{
    // for non-negative doubles the IEEE bit pattern orders like the value
    atomicMax(reinterpret_cast<unsigned long long*>(addr), static_cast<unsigned long long>(__double_as_longlong(fabs(v))));
}

// the end of every solve kernel: a singular system is flagged; otherwise maxRelChange = max(maxRelChange, change.max()) with
// Python's builtin max (rh_method.py:741) -- a NaN never replaces the running maximum, so a depth whose change is NaN drops out
__device__ __forceinline__ void record_solve(bool solved, double change, unsigned long long* singular, double* dPcol, int col,
                                             int atom, int k, int Ns)
{
    if (!solved) flag_singular(singular, col, atom, k, Ns);
    else if (change == change) atomic_max_nonneg(&dPcol[col], change);
}

} // namespace lsxd
