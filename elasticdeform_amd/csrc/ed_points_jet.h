// ed_points_jet.h -- the calls of deform_points_jet.hip as the entry points hand them to its launchers: the coordinate
// map r(q) at real positions with its first and second derivatives J = dr/dq, H = d^2r/dq dq, and the adjoint of the
// three.  Notation: the head of deform_points_jet.hip.
#pragma once

#include "ed_params.h"

namespace ed {

// r, J and H at the points: one thread per point, blockIdx.y = sample, fp64; no scratch, no atomics, no
// synchronisation.  1 to 3 deformed axes and at most 65535 samples; hipErrorNotSupported (nothing launched) otherwise.
struct PointsJetCall {
    GridGeom g;                   // g.disp: the prefiltered grid of sample 0; in_len >= 2 on every axis
    int nbatch;
    int64_t npts;
    int64_t disp_bstride;
    BatchArray pts;               // (npts, naxis) float32 / float64 (read)
    BatchArray res;               // (npts, naxis) float32 / float64
    BatchArray jac;               // float64 (npts, naxis, naxis); may be empty
    BatchArray hess;              // float64 (npts, naxis, naxis, naxis); may be empty: the second-derivative sweep is skipped
};
hipError_t launch_deform_points_derivatives(const PointsJetCall& c, hipStream_t stream);

// The adjoint for the cotangents u = dL/dr, A = dL/dJ, G = dL/dH (any of them empty): the per-point rows dL/dq, the
// gradient with respect to the prefiltered grid and with respect to the inverse map K.  The sums go through the
// fixed-point reduction of ed_points_grad.h (order-independent bits), with its rule of own bounds: each of the two
// quanta has a state of its own.  The call clears its scratch itself: [per sample kGradHead words | per sample
// naxis (naxis + 1) + naxis prod ncp cells] and no u rows, points_jet_scratch_bytes() bytes from the caller.  Four
// launches.
struct PointsJetGradCall {
    GridGeom g;
    int nbatch;
    int64_t npts;
    int64_t disp_bstride;
    BatchArray pos;               // (npts, naxis) float32 / float64: q (read)
    BatchArray du;                // (npts, naxis) float32 / float64 (read); may be empty
    BatchArray dA;                // (npts, naxis, naxis) float32 / float64 (read); may be empty
    BatchArray dG;                // (npts, naxis, naxis, naxis) float32 / float64 (read); may be empty
    BatchArray dpts;              // (npts, naxis) float32 / float64; may be empty
    BatchArray ddisp;             // the grid's shape, a floating dtype; may be empty
    BatchArray dK;                // float64 (naxis, naxis + 1); may be empty
    char* scratch;
};
size_t points_jet_scratch_bytes(const GridGeom& g, int nbatch);
hipError_t launch_deform_points_derivatives_gradient(const PointsJetGradCall& c, hipStream_t stream);

}  // namespace ed
