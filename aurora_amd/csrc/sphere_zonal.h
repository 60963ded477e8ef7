// The zonal stage of the spherical-harmonic analysis as a launch that two translation units issue: sphere_spectra.hip, which
// holds the kernel (sphere_zonal_kernel), and sphere_transform.hip, whose analysis starts with the same launch without a
// truth.  One copy of the kernel in the library; the callers have checked the arguments.
#pragma once
#include "common.h"

namespace aurora {

// F_m(i) of every plane (and of its truth, where truth_planes is not null) into F -- pairs of doubles, [plane][field][m][i] of
// sphere_spectra_index.h -- and the (plane, row chunk) flag words into `flags`; returns check_launch's code.
int sphere_zonal_launch(const float* const* pred_planes, const float* const* truth_planes, int n_planes, int n_lat, int n_lon,
                        int lmax, int pole_rows, const double* twiddle, void* F, int* flags, hipStream_t s);

}  // namespace aurora
