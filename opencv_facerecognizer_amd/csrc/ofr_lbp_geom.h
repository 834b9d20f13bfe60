// ExtendedLBP sampling geometry shared by the byte kernels (ofr_lbp.hip) and the float kernels
// (ofr_lbp_float.hip): the kernel-argument form of the host's (offsets, weights) and the compiled
// radius-1, 8-neighbour special case.
#pragma once
#include <cstdlib>

#include "ofr_common.h"

namespace ofr {

constexpr int MAXP = 32;

struct LbpGeom {
  int P;
  int H, W, dy, dx;   // image and code-image sizes
  int oy, ox;         // centre offset
  int nterm[MAXP];    // non-zero terms per point (1..4)
  int toff[MAXP][4];  // pixel offset (ty*W + tx) of each term, relative to the code pixel's block origin
  double tw[MAXP][4]; // weight of each term
};

// ExtendedLBP(radius=1, neighbors=8): which cell of the 3x3 block each term reads, and which weights are
// zero.  The weights themselves are the caller's (bits 4 and 6 carry the 2^-53 / 2^-52 terms of np.sin /
// np.cos).
struct R1P8 {
  double w[8][4];
};
constexpr int R1P8_OFFS[8][4] = {{1, 2, 1, 2}, {0, 1, 1, 2}, {0, 1, 0, 1}, {0, 0, 1, 1},
                                 {0, 0, 1, 0}, {1, 0, 2, 1}, {2, 0, 2, 1}, {1, 1, 2, 2}};
// non-zero terms per point: bit t set = weight t non-zero (points 0 and 2: weight 1.0 alone)
constexpr int R1P8_TERMS[8] = {0x1, 0xf, 0x1, 0xf, 0x5, 0xf, 0x3, 0xf};

// the caller's geometry is the compiled r1p8 one: same offsets, same zero pattern, weight 1.0 alone
// for points 0 and 2
static inline bool r1p8_match(int P, const int32_t* offs, const double* w, int oy, int ox, int by, int bx, R1P8& k) {
  if (P != 8 || oy != 1 || ox != 1 || by != 3 || bx != 3) return false;
  for (int i = 0; i < 8; ++i)
    for (int t = 0; t < 4; ++t) {
      if (offs[4 * i + t] != R1P8_OFFS[i][t]) return false;
      const double wt = w[4 * i + t];
      if (((R1P8_TERMS[i] >> t) & 1) != (wt != 0.0 ? 1 : 0)) return false;
      k.w[i][t] = wt;
    }
  return w[0] == 1.0 && w[8] == 1.0;
}

static inline bool lbp_generic_forced() {
  static const bool f = [] {
    const char* e = getenv("OFR_LBP_GENERIC");
    return e && atoi(e) != 0;
  }();
  return f;
}

static inline int make_geom(LbpGeom& g, int H, int W, int P, const int32_t* offs, const double* w, int oy, int ox,
                            int by, int bx) {
  if (P < 1 || P > MAXP) return fail(OFR_E_UNSUPPORTED, "ofr_elbp: neighbors must be in [1, 32]");
  if (!offs || !w) return fail(OFR_E_INVALID, "ofr_elbp: null geometry");
  g.P = P;
  g.H = H;
  g.W = W;
  g.dy = H - by + 1;
  g.dx = W - bx + 1;
  g.oy = oy;
  g.ox = ox;
  for (int i = 0; i < P; ++i) {
    // (fy, fx), (fy, cx), (cy, fx), (cy, cx) with weights w1..w4 (lbp.py:123-126)
    const int fy = offs[4 * i + 0], fx = offs[4 * i + 1], cy = offs[4 * i + 2], cx = offs[4 * i + 3];
    if (fy < 0 || fx < 0 || cy >= by || cx >= bx || cy < fy || cx < fx)
      return fail(OFR_E_INVALID, "ofr_elbp: sample offsets outside the block");
    const int pos[4][2] = {{fy, fx}, {fy, cx}, {cy, fx}, {cy, cx}};
    int nt = 0;
    for (int t = 0; t < 4; ++t) {
      const double wt = w[4 * i + t];
      if (!(wt >= 0.0)) return fail(OFR_E_INVALID, "ofr_elbp: negative or NaN weight");
      if (wt == 0.0) continue;  // exact +0 contribution
      g.toff[i][nt] = pos[t][0] * W + pos[t][1];
      g.tw[i][nt] = wt;
      ++nt;
    }
    if (nt == 0) {  // all-zero weights: N = 0
      g.toff[i][0] = 0;
      g.tw[i][0] = 0.0;
      nt = 1;
    }
    g.nterm[i] = nt;
  }
  return OFR_OK;
}

}  // namespace ofr
