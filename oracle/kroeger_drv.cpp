// kroeger_drv.cpp -- extern "C" driver of the reference's own LK / densification / scale-loop code (kroeger/oflow.cpp,
// patch.cpp, patchgrid.cpp, refine_variational.cpp, compiled unmodified against oracle/eigen_min by `make -C oracle ref`).
// TEST INFRASTRUCTURE ONLY: loaded by oracle/kroeger_ref.py to pin oracle/dis_oracle.c's restatement bit for bit.
//
// The pyramids come from the oracle (dis_pyramid_build: run_dense.cpp's OpenCV pyramid, padding and Sobel restated), so the
// pin covers everything OFClass does on them, not the pyramid itself.
#include <iostream>
#include <vector>
#include <cmath>
#include <cstring>

#include <Eigen/Core>
#include <Eigen/LU>
#include <Eigen/Dense>

#include "oflow.h"
#include "dis_oracle.h"

#ifndef SELECTMODE
#error "SELECTMODE (1 optical flow, 2 depth) must be set as for the reference build"
#endif
#ifndef SELECTCHANNEL
#error "SELECTCHANNEL (1 gray, 3 RGB) must be set as for the reference build"
#endif

namespace {

// one OFClass construction (oflow.cpp:32-363) over levels sc_f .. sc_l of the two pyramids -> flow of level sc_l
void run_ofclass(const dis_pyramid *P0, const dis_pyramid *P1, const dis_params *p, int sc_f, int sc_l, bool usetvref,
                 const float *initflow, float *out)
{
  const int n = P0->nlev;
  std::vector<const float *> a(n), ax(n), ay(n), b(n), bx(n), by(n);
  for (int l = 0; l < n; ++l) {
    a[l] = P0->im[l]; ax[l] = P0->dx[l]; ay[l] = P0->dy[l];
    b[l] = P1->im[l]; bx[l] = P1->dx[l]; by[l] = P1->dy[l];
  }
  OFC::OFClass ofc(a.data(), ax.data(), ay.data(), b.data(), bx.data(), by.data(), p->ps, out, initflow, P0->w0, P0->h0,
                   sc_f, sc_l, p->max_iter, p->min_iter, p->dp_thresh, p->dr_thresh, p->res_thresh, p->ps, p->patove,
                   p->usefbcon != 0, p->costfct, p->noc, p->patnorm, usetvref, p->tv_alpha, p->tv_gamma, p->tv_delta,
                   p->tv_innerit, p->tv_solverit, p->tv_sor, 0);
  (void)ofc;
}

}  // namespace

extern "C" {

// which build this is: SELECTMODE * 10 + SELECTCHANNEL
int kroeger_build_mode() { return SELECTMODE * 10 + SELECTCHANNEL; }

// OFClass on prebuilt pyramids -> finest-level flow (h_l x w_l x nch, nch = 2, or 1 for depth), like dis_flow_pyr.
// level_dump (optional): for l = sc_f .. sc_l the flow of level l before and after its refinement, concatenated, in the layout
// of dis_flow_pyr's dump.  OFClass returns only its last level, so level l "after" is a run with sc_l = l (the forward flow of
// level l does not depend on the levels below it), and "before" a run over level l alone with usetvref off, started from the
// "after" flow of level l + 1 (or initflow) through the same InitializeFromCoarserOF.  With usefbcon and usetvref both on,
// that restart cannot reproduce the backward grid's start, so "before" is filled with NaN.
// Returns 0, or -1 when p does not match this build (depth / noc) or normoutlier differs from oflow.h's fixed 5.
int kroeger_flow_pyr(const dis_pyramid *P0, const dis_pyramid *P1, const dis_params *p, const float *initflow, float *outflow,
                     float *level_dump)
{
  if ((p->depth ? 2 : 1) != SELECTMODE || p->noc != SELECTCHANNEL || p->normoutlier != 5.0f) return -1;
  const int nch = SELECTMODE == 1 ? 2 : 1;
  run_ofclass(P0, P1, p, p->sc_f, p->sc_l, p->usetvref != 0, initflow, outflow);
  if (!level_dump) return 0;
  size_t off = 0;
  const float *coarser = initflow;
  for (int sl = p->sc_f; sl >= p->sc_l; --sl) {
    const size_t n = (size_t)nch * (P0->w0 >> sl) * (P0->h0 >> sl);
    float *pre = level_dump + off, *post = level_dump + off + n;
    run_ofclass(P0, P1, p, p->sc_f, sl, p->usetvref != 0, initflow, post);
    if (!p->usetvref) std::memcpy(pre, post, sizeof(float) * n);
    else if (!p->usefbcon) run_ofclass(P0, P1, p, sl, sl, false, coarser, pre);
    else for (size_t i = 0; i < n; ++i) pre[i] = NAN;
    coarser = post;
    off += 2 * n;
  }
  return 0;
}

}  // extern "C"
