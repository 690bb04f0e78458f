/* alignn_thermo.h - the entry points of libalignn_hip.so for harmonic thermodynamics and the quasi-harmonic approximation
 * (csrc/thermo.hip; alignn_amd/thermo.py is the driver and binds this header, tests/thermo_ref.py the numpy restatement).
 *
 * A header of its own beside alignn_hip.h, in the same regular form (one extern "C" block, prototypes over the base types, no
 * structs): alignn_amd/_abi.py reads both.  Every pointer is a device pointer unless it is called a workspace size; `stream` is
 * a hipStream_t.  Every entry point returns 0 or the HIP error; hipErrorInvalidValue (1) for an argument out of its range.
 *
 * float64 without contraction, no atomics, every sum in a fixed order that depends on the structure's own data only: a
 * structure's bits do not depend on the launch it is in, nor on its place in it.
 */
#ifndef ALIGNN_THERMO_H
#define ALIGNN_THERMO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * _phonon_thermal: the sums over the phonon modes of a q-mesh (phonopy's run_thermal_properties), per primitive cell.
 *
 *   freqs          the mesh frequencies (eV) of all structures, flat, imaginary modes negative: the layout of alignn_phonon_dos
 *   freq_off       [n_structures + 1] structure s owns freqs [freq_off[s], freq_off[s + 1]): n_q[s] q-points x its 3n modes
 *   n_q            [n_structures] the number of q-points of structure s (the sums are averages over them), >= 1
 *   n_structures   1 .. 65535
 *   max_freqs      the largest freq_off[s + 1] - freq_off[s] (sizes the launch and the workspace)
 *   temperatures   [n_temps] K, finite and >= 0
 *   n_temps        >= 1
 *   cutoff         eV, >= 0: a mode eps counts only if eps > cutoff; every other mode (imaginary, zero, at the cutoff) is skipped
 *   workspace      at least _phonon_thermal_workspace(n_structures, max_freqs, n_temps) bytes: the partial sums [chunk][n_temps][4]
 *                  of every chunk of 1024 frequencies; the chunk size does not depend on the batch
 *   workspace_bytes  its size
 *   free_energy, internal_energy, entropy, heat_capacity   [n_structures][n_temps] eV, eV, eV/K, eV/K
 *   zpe            [n_structures] eV
 *   n_skipped      [n_structures] the modes of the mesh that were not counted
 *
 * kB = 1.38064852e-23 / 1.6021766208e-19 eV/K (CODATA 2014).  For T > 0, with x = eps / (kB T), em = exp(-x), om = -expm1(-x),
 * over the counted modes and divided by n_q:
 *   F = sum eps / 2 + kB T log(om)        U = sum eps (1 / 2 + em / om)
 *   S = kB sum (x / om) em - log(om)      Cv = kB sum (x / om)^2 em       zpe = sum eps / 2
 * A mode with x > 700, and every mode at T = 0, contributes its T -> 0 limit (eps / 2 to F and U, nothing to S and Cv), so
 * F = U = zpe bit for bit and S = Cv = 0 at T = 0.  One workgroup per (chunk, structure) holds its frequencies in registers and
 * loops over the temperatures; a second launch adds a structure's chunks in ascending order.
 * ------------------------------------------------------------------------------------------ */
size_t alignn_phonon_thermal_workspace(int n_structures, int64_t max_freqs, int n_temps);
int alignn_phonon_thermal(const double* freqs, const int64_t* freq_off, const int32_t* n_q, int n_structures, int64_t max_freqs,
                          const double* temperatures, int n_temps, double cutoff, void* workspace, size_t workspace_bytes,
                          double* free_energy, double* internal_energy, double* entropy, double* heat_capacity, double* zpe,
                          int32_t* n_skipped, void* stream);

/* ------------------------------------------------------------------------------------------
 * _qha_derive: the thermal quantities of the quasi-harmonic approximation from the per-temperature equation-of-state fits of
 * E(V) + F_phonon(V, T) (alignn_eos_fit on n_structures x n_temps rows).  One wavefront per (structure, temperature i), one
 * lane per volume point.
 *
 *   volumes        [n_structures][n_points] the volumes of the strained cells (A^3)
 *   heat_capacity  [n_structures][n_points][n_temps] Cv of _phonon_thermal at every volume (eV/K)
 *   entropy        [n_structures][n_points][n_temps] S likewise
 *   temperatures   [n_temps] K, strictly increasing
 *   v_eq           [n_structures][n_temps] the fitted equilibrium volume V_i
 *   b_t            [n_structures][n_temps] the fitted isothermal bulk modulus B_i (eV/A^3)
 *   status         [n_structures][n_temps] the fit's status (2: no fit)
 *   n_structures   0 .. 65535
 *   n_points       4 .. 64
 *   n_temps        >= 1
 *   alpha          [n_structures][n_temps] the volumetric thermal expansion (1/K): (V_{i+1} - V_{i-1}) / (T_{i+1} - T_{i-1}) / V_i
 *                  inside, the one-sided difference to the neighbour at the two ends, NaN when n_temps = 1
 *   cv_out, s_out  [n_structures][n_temps] Cv and S at V_i: the least-squares quadratic in x = (V - mid) / h over the points
 *                  (mid = (Vmax + Vmin) / 2, h = (Vmax - Vmin) / 2; 3 x 3 normal equations by Cholesky) evaluated at x(V_i)
 *   cp_out         [n_structures][n_temps] C_p = Cv_i + T_i V_i alpha_i^2 B_i (eV/K)
 *   gamma          [n_structures][n_temps] the thermodynamic Grueneisen parameter alpha_i B_i V_i / Cv_i, NaN where Cv_i = 0
 *   inside         [n_structures][n_temps] 1 where Vmin <= V_i <= Vmax, else 0
 *
 * Where status_i = 2 every output of i is NaN (inside 0); where a neighbour that alpha_i needs has status 2, alpha_i and what
 * is formed from it (cp_out, gamma) are NaN.
 * ------------------------------------------------------------------------------------------ */
int alignn_qha_derive(const double* volumes, const double* heat_capacity, const double* entropy, const double* temperatures,
                      const double* v_eq, const double* b_t, const int32_t* status, int n_structures, int n_points, int n_temps,
                      double* alpha, double* cv_out, double* s_out, double* cp_out, double* gamma, int32_t* inside, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNN_THERMO_H */
