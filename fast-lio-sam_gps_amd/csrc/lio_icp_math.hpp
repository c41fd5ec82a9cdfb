// lio_icp_math.hpp — the loop ICP's host arithmetic (lio_icp_math.cpp): the two Umeyamas, the composition of
// the final transform and PCL's convergence criteria.  Pure functions, no HIP.
#pragma once
#include "../../include/lio_gpu.h"

namespace lio::icp {

// Umeyama without scaling (Eigen::umeyama(src, dst, false)) from the double statistics:
// st[0]=n, st[1..3]=sum p, st[4..6]=sum q, st[7..15]=sum q p^T, all about c0.  Ti: row-major 4x4.
void umeyama(const double* st, const double c0[3], float Ti[16]);

// pcl::umeyama(src, dst, false) in float from the fidelity statistics (out16: the float sums, the count's bits
// in [6], sigma in [7..15]): order 1 takes the raw sequential sigma accumulator (scaled here), orders 2 / 3 sigma
// as Eigen's GEMM leaves it
void umeyama_pcl_float(const float* out16, float Ti[16], int order = 1);

// fin = Ti * fin (row-major 4x4 float; each entry summed in column order as Eigen's Matrix4f product does)
void compose4f(const float Ti[16], float fin[16]);

// pcl::registration::DefaultConvergenceCriteria<float> (PCL 1.10, max_iterations_similar_transforms_ = 0)
// after the iteration that produced the incremental transform Ti and the mean squared error mse; `iters`
// counts that iteration.  True: the loop ends, *state is the criterion that ended it (1 iterations, 2
// transform, 3 absolute MSE, 4 relative MSE).  False: *state is left alone.
bool convergence_step(const float Ti[16], double mse, double prev_mse, int iters, const lio_icp_params& p, int* state);

}  // namespace lio::icp
