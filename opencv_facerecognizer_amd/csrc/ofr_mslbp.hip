// Multi-scale LBP histograms on gfx950 (bit-exact): the feature rows of
//   CombineOperator(SpatialHistogram(ExtendedLBP(r_0, P), sz), SpatialHistogram(ExtendedLBP(r_1, P), sz), ...)
// for S = 2..4 scales that share P <= 8 and the grid, in ONE launch: every scale's per-cell counts and /
// or the fp32 density rows in the operator's own order (scale-major, cells row-major, bins).
//
// Semantics per scale are ofr_lbp.hip's (uint8 images) and ofr_lbp_float.hip's (float32 / float64 images):
// fp64 products and sums in the order of lbp.py:123-126, zero weights dropped on the host, no contraction,
// bit i = N >= C with C the uint8 centre (centre_u8() of a float pixel).  A row value is
// (float)((double)count / (double)(py_s * px_s)): the float32 rounding of the reference's float64 feature,
// as ofr_hist_density_f32 forms it.
//
// Design.
// * One staging for all scales.  A 1024-thread workgroup owns (image, band of cell rows).  The scales cut
//   the same grid out of code images of different sizes, so cell row c of scale s starts at pixel row
//   c * py_s: the band stages, once, the contiguous pixel rows from min_s(cr0 * py_s) to
//   max_s(cr1 * py_s + by_s - 1), and scale s walks the plane from its own first row.  Bytes stay bytes:
//   the plane sits in LDS at the same offset inside a 16-byte line as the band's first byte in memory,
//   so everything between the first and the last 16-byte boundary moves as 16-byte loads and stores,
//   whatever the row pitch.  float32 / float64 pixels become fp64 once, in lbpf::stage_plane.
//   Then all threads walk scale 0's code pixels, then scale 1's, ...: the plane is read-only and the
//   scales' counters are disjoint, so there is NO barrier between scales -- one after staging, one before
//   the flush.
// * Packed 16-bit LDS counters.  Every cell holds at most 65535 code pixels, so two bins share one u32:
//   atomicAdd(&h[bin >> 1], 1u << (16 * (bin & 1))); the low half can never carry into the high one.
//   Half the footprint of the u32 counters of the single-scale kernels: that is what lets S scales share
//   a band.  128 x 128 bytes, 8 x 8 cells, 256 bins, 3 scales: 96 KiB counters + 16 KiB image in one
//   band, run as two bands of about 57 KiB.
// * Work split.  The fewest bands whose evened-out cell rows fit 80 KiB (counters + plane of the band
//   that needs most), else 160 KiB.  Bands write disjoint outputs.  No global-atomics form: when one cell
//   row of all scales does not fit 160 KiB the call is OFR_E_UNSUPPORTED.
// * Lanes.  Per scale the strip map of the float kernels: nstrips = 1024 / width, thread i takes column
//   i % width of strip i / width (the widths differ per scale).  A scale whose geometry is the compiled
//   radius-1, 8-neighbour one walks down its column with the 3 x 3 block in nine fp64 registers; any
//   other scale reads its terms from the plane, RB pixels of the column per pass of the points (offsets
//   and weights are kernel arguments: a compact 440-byte struct per scale, sized for P <= 8).
// * Flush.  A counter pair already is the 32-bit word of two uint16 counts; the rows leave as 16-byte
//   stores (2^P >= 4, ld a multiple of 4).  Band 0 zeroes the row's padding.
#include <climits>

#include "ofr_common.h"
#include "ofr_lbp_band.h"
#include "ofr_lbp_geom.h"

#pragma clang fp contract(off)

namespace ofr {
namespace mslbp {

using lbpf::LDS_HALF;
using lbpf::LDS_MAX;
using lbpf::THREADS;

constexpr int MAX_SCALES = 4;
constexpr int MAX_POINTS = 8;
constexpr int RB = 4;  // code pixels a lane of a generic scale carries through the points at a time

struct Scale {
  int py, px;  // cell size in code pixels
  int halo;    // by - 1: pixel rows below a code row
  int coff;    // centre offset oy*W + ox
  int r1p8;    // the compiled 3 x 3 form: tw then holds the caller's four weights per point, zeros included
  int nterm[MAX_POINTS];
  int toff[MAX_POINTS][4];
  double tw[MAX_POINTS][4];
};

static_assert(sizeof(Scale) == 440, "four of them and the header stay far below the 4 KiB of kernel arguments");

struct Args {
  int H, W, S, nb_log2;
  int gr, gc;
  int rows, nbands;  // cell rows per band
  int64_t ld;
  Scale sc[MAX_SCALES];
};

// `count` bytes whose source and destination share their offset inside a 16-byte line
__device__ __forceinline__ void stage_bytes(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int count) {
  const int head = min(count, (int)((16u - (unsigned)((uintptr_t)src & 15u)) & 15u));
  const int nvec = (count - head) >> 4;
  for (int i = threadIdx.x; i < head; i += THREADS) dst[i] = src[i];
  const uint4* body = reinterpret_cast<const uint4*>(src + head);
  uint4* out = reinterpret_cast<uint4*>(dst + head);
  for (int i = threadIdx.x; i < nvec; i += THREADS) out[i] = body[i];
  for (int i = head + 16 * nvec + threadIdx.x; i < count; i += THREADS) dst[i] = src[i];
}

template <typename T>
__device__ __forceinline__ double centre_of(double x) {
  if constexpr (sizeof(T) == 1) return x;  // a byte is its own uint8 centre
  else return lbpf::centre_u8(x);
}

__device__ __forceinline__ void count_code(uint32_t* h, int idx) { atomicAdd(&h[idx >> 1], 1u << (16 * (idx & 1))); }

// T: the plane's element, uint8_t (byte images) or double (float32 / float64 images, staged as fp64)
template <typename T>
__global__ void __launch_bounds__(THREADS) mslbp_kernel(const void* __restrict__ imgs, int pixel_bytes, Args a,
                                                        uint32_t* __restrict__ counts, float* __restrict__ rows) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hist[];
  const int64_t img = blockIdx.x / a.nbands;
  const int band = blockIdx.x - (int)img * a.nbands;
  const int cr0 = band * a.rows, cr1 = min(a.gr, cr0 + a.rows);
  const int nb = 1 << a.nb_log2;
  const int W = a.W;
  const int cw = a.rows * a.gc * (nb >> 1);        // counter words per scale: two bins per word
  const int nwords = (int)round_up(a.S * cw, 4);
  int r_lo = INT_MAX, r_hi = 0;                    // the pixel rows any scale of the band touches
  for (int s = 0; s < a.S; ++s) {
    r_lo = min(r_lo, cr0 * a.sc[s].py);
    r_hi = max(r_hi, cr1 * a.sc[s].py + a.sc[s].halo);
  }
  for (int i = threadIdx.x; i < nwords / 4; i += THREADS) reinterpret_cast<uint4*>(hist)[i] = make_uint4(0, 0, 0, 0);
  const int64_t first_px = (img * a.H + r_lo) * (int64_t)W;
  const int npx = (r_hi - r_lo) * W;
  const T* im;
  if constexpr (sizeof(T) == 1) {
    const uint8_t* src = reinterpret_cast<const uint8_t*>(imgs) + first_px;
    uint8_t* dst = reinterpret_cast<uint8_t*>(hist + nwords) + ((uintptr_t)src & 15u);
    stage_bytes(src, dst, npx);
    im = dst;
  } else {
    double* dst = reinterpret_cast<double*>(hist + nwords);
    if (pixel_bytes == 4) lbpf::stage_plane(reinterpret_cast<const float*>(imgs) + first_px, dst, npx);
    else lbpf::stage_plane(reinterpret_cast<const double*>(imgs) + first_px, dst, npx);
    im = dst;
  }
  __syncthreads();
  for (int s = 0; s < a.S; ++s) {
    const Scale& sc = a.sc[s];
    uint32_t* h = hist + s * cw;
    const T* pl = im + (cr0 * sc.py - r_lo) * W;  // the scale's first code row of the band
    const int hpx = (cr1 - cr0) * sc.py;          // code rows of the band
    const int wpx = a.gc * sc.px;                 // covered code columns
    const int nstrips = max(1, min(hpx, THREADS / wpx));
    const int srows = (hpx + nstrips - 1) / nstrips;
    for (int item = threadIdx.x; item < nstrips * wpx; item += THREADS) {
      const int strip = item / wpx, x = item - strip * wpx;
      const int ya = strip * srows, yb = min(hpx, ya + srows);
      if (ya >= yb) continue;
      const int cxo = x / sc.px;
      int cyc = ya / sc.py, ry = ya - cyc * sc.py;
      const T* col = pl + x;
      if (sc.r1p8) {
        double b00 = col[ya * W], b01 = col[ya * W + 1], b02 = col[ya * W + 2];
        double b10 = col[(ya + 1) * W], b11 = col[(ya + 1) * W + 1], b12 = col[(ya + 1) * W + 2];
        for (int y = ya; y < yb; ++y) {
          const T* r2 = col + (y + 2) * W;
          const double b20 = r2[0], b21 = r2[1], b22 = r2[2];
          const double C = centre_of<T>(b11);
          uint32_t code = 0;
          double N;
          N = sc.tw[0][0] * b12;
          code |= (N >= C ? 1u : 0u) << 0;
          N = sc.tw[1][0] * b01; N = N + sc.tw[1][1] * b02; N = N + sc.tw[1][2] * b11; N = N + sc.tw[1][3] * b12;
          code |= (N >= C ? 1u : 0u) << 1;
          N = sc.tw[2][0] * b01;
          code |= (N >= C ? 1u : 0u) << 2;
          N = sc.tw[3][0] * b00; N = N + sc.tw[3][1] * b01; N = N + sc.tw[3][2] * b10; N = N + sc.tw[3][3] * b11;
          code |= (N >= C ? 1u : 0u) << 3;
          N = sc.tw[4][0] * b00; N = N + sc.tw[4][2] * b10;
          code |= (N >= C ? 1u : 0u) << 4;
          N = sc.tw[5][0] * b10; N = N + sc.tw[5][1] * b11; N = N + sc.tw[5][2] * b20; N = N + sc.tw[5][3] * b21;
          code |= (N >= C ? 1u : 0u) << 5;
          N = sc.tw[6][0] * b20; N = N + sc.tw[6][1] * b21;
          code |= (N >= C ? 1u : 0u) << 6;
          N = sc.tw[7][0] * b11; N = N + sc.tw[7][1] * b12; N = N + sc.tw[7][2] * b21; N = N + sc.tw[7][3] * b22;
          code |= (N >= C ? 1u : 0u) << 7;
          count_code(h, (cyc * a.gc + cxo) * nb + (int)code);
          if (++ry == sc.py) {
            ry = 0;
            ++cyc;
          }
          b00 = b10; b01 = b11; b02 = b12;
          b10 = b20; b11 = b21; b12 = b22;
        }
      } else {
        // points outer, RB pixels of the column inner: every (weight, offset) is one scalar load per RB
        // pixels, and the atomics go out after all codes of the group (a scalar load's wait would drain them)
        for (int y0 = ya; y0 < yb; y0 += RB) {
          uint32_t code[RB];
          double C[RB], N[RB];
          int base[RB];
#pragma unroll
          for (int r = 0; r < RB; ++r) {
            base[r] = min(y0 + r, yb - 1) * W;
            C[r] = centre_of<T>((double)col[base[r] + sc.coff]);
            code[r] = 0;
          }
          for (int i = 0; i < a.nb_log2; ++i) {
            const int nt = sc.nterm[i];
            {
              const int off = sc.toff[i][0];
              const double wt = sc.tw[i][0];
#pragma unroll
              for (int r = 0; r < RB; ++r) N[r] = wt * (double)col[base[r] + off];
            }
            for (int t = 1; t < nt; ++t) {  // lbp.py:123-126 order, no contraction
              const int off = sc.toff[i][t];
              const double wt = sc.tw[i][t];
#pragma unroll
              for (int r = 0; r < RB; ++r) {
                const double prod = wt * (double)col[base[r] + off];
                N[r] = N[r] + prod;
              }
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) code[r] |= (N[r] >= C[r] ? 1u : 0u) << i;
          }
#pragma unroll
          for (int r = 0; r < RB; ++r) {
            if (y0 + r < yb) {
              count_code(h, (cyc * a.gc + cxo) * nb + (int)code[r]);
              if (++ry == sc.py) {
                ry = 0;
                ++cyc;
              }
            }
          }
        }
      }
    }
  }
  __syncthreads();
  // flush: four bins (two counter words) per thread and pass
  const int64_t cells = (int64_t)a.gr * a.gc;
  const int64_t row_bins = a.S * cells * nb;
  const int quads = (cr1 - cr0) * a.gc * (nb >> 2);
  float* row = rows ? rows + img * a.ld : nullptr;
  for (int s = 0; s < a.S; ++s) {
    const uint2* h = reinterpret_cast<const uint2*>(hist + s * cw);
    const double cell = (double)(a.sc[s].py * a.sc[s].px);
    const int64_t first = (s * cells + (int64_t)cr0 * a.gc) * nb;  // the band's first bin of this scale in the row
    for (int i = threadIdx.x; i < quads; i += THREADS) {
      const uint2 v = h[i];
      if (counts) {
        uint32_t* o = counts + ((img * row_bins + first) >> 1) + 2 * i;
        o[0] = v.x;
        o[1] = v.y;
      }
      if (row) {
        float4 d;
        d.x = (float)((double)(v.x & 0xffffu) / cell);
        d.y = (float)((double)(v.x >> 16) / cell);
        d.z = (float)((double)(v.y & 0xffffu) / cell);
        d.w = (float)((double)(v.y >> 16) / cell);
        *reinterpret_cast<float4*>(row + first + 4 * i) = d;
      }
    }
  }
  if (row && band == 0)
    for (int64_t j = row_bins + threadIdx.x; j < a.ld; j += THREADS) row[j] = 0.0f;
}

// LDS bytes of a launch with `rows` cell rows per band: counters of all scales + the plane of the band
// that touches most pixel rows (bytes: 16 more, the plane keeps its source's offset in a 16-byte line)
static int64_t lds_bytes(const Args& a, int rows, int plane_bytes) {
  const int64_t counters = round_up((int64_t)a.S * rows * a.gc * ((1LL << a.nb_log2) / 2), 4) * 4;
  int64_t px_rows = 0;
  for (int cr0 = 0; cr0 < a.gr; cr0 += rows) {
    const int cr1 = std::min(a.gr, cr0 + rows);
    int64_t lo = INT_MAX, hi = 0;
    for (int s = 0; s < a.S; ++s) {
      lo = std::min<int64_t>(lo, (int64_t)cr0 * a.sc[s].py);
      hi = std::max<int64_t>(hi, (int64_t)cr1 * a.sc[s].py + a.sc[s].halo);
    }
    px_rows = std::max(px_rows, hi - lo);
  }
  const int64_t plane = px_rows * a.W * plane_bytes;
  return counters + (plane_bytes == 1 ? round_up(plane, 16) + 16 : plane);
}

template <typename T>
static int launch(hipStream_t st, const void* imgs, int pixel_bytes, int64_t n, const Args& a, size_t lds,
                  uint32_t* counts, float* rows) {
  // on every launch: the attribute belongs to the current device, and the call is cheap
  hipError_t e = hipFuncSetAttribute((const void*)mslbp_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
  if (e != hipSuccess) return hip_status(e, "hipFuncSetAttribute(mslbp_kernel)");
  hipLaunchKernelGGL(mslbp_kernel<T>, dim3((unsigned)(n * a.nbands)), dim3(THREADS), lds, st, imgs, pixel_bytes, a,
                     counts, rows);
  OFR_LAUNCH_CHECK("mslbp_kernel");
  return OFR_OK;
}

}  // namespace mslbp
}  // namespace ofr

using namespace ofr;
using namespace ofr::mslbp;

extern "C" int ofr_mslbp_hist(void* stream, const void* imgs, int pixel_bytes, int64_t n, int H, int W, int S, int P,
                              const int32_t* offs, const double* w, const int32_t* block, int gr, int gc,
                              uint16_t* counts, float* rows, int64_t ld) {
  const std::string who("ofr_mslbp_hist");
  OFR_CHECK_ARG(n >= 0 && H >= 1 && W >= 1 && gr >= 1 && gc >= 1, "ofr_mslbp_hist: bad sizes");
  OFR_CHECK_ARG(pixel_bytes == 1 || pixel_bytes == 4 || pixel_bytes == 8,
                "ofr_mslbp_hist: pixel_bytes must be 1 (uint8), 4 (float32) or 8 (float64)");
  if (S < 2 || S > MAX_SCALES) return fail(OFR_E_UNSUPPORTED, who + ": 2 to 4 scales");
  if (P < 2 || P > MAX_POINTS) return fail(OFR_E_UNSUPPORTED, who + ": neighbors must be in [2, 8]");
  if ((int64_t)H * W > 0x7fffffffLL / 8) return fail(OFR_E_UNSUPPORTED, who + ": image too large");
  OFR_CHECK_ARG(offs && w && block, "ofr_mslbp_hist: null geometry");
  OFR_CHECK_ARG(counts || rows, "ofr_mslbp_hist: neither counts nor rows asked for");
  Args a = {};
  a.H = H;
  a.W = W;
  a.S = S;
  a.nb_log2 = P;
  a.gr = gr;
  a.gc = gc;
  a.ld = ld;
  for (int s = 0; s < S; ++s) {
    const int32_t* so = offs + (size_t)s * P * 4;
    const double* sw = w + (size_t)s * P * 4;
    const int oy = block[4 * s], ox = block[4 * s + 1], by = block[4 * s + 2], bx = block[4 * s + 3];
    OFR_CHECK_ARG(by >= 1 && bx >= 1 && oy >= 0 && ox >= 0 && oy < by && ox < bx,
                  "ofr_mslbp_hist: centre outside the block");
    LbpGeom g;
    const int rc = make_geom(g, H, W, P, so, sw, oy, ox, by, bx);
    if (rc) return rc;
    Scale& sc = a.sc[s];
    sc.py = g.dy > 0 ? g.dy / gr : 0;
    sc.px = g.dx > 0 ? g.dx / gc : 0;
    const int64_t cell = (int64_t)sc.py * sc.px;
    if (cell < 1 || cell > 65535)
      return fail(OFR_E_UNSUPPORTED, who + ": every scale's cell must hold 1 to 65535 code pixels");
    sc.halo = by - 1;
    sc.coff = oy * W + ox;
    R1P8 k = {};
    sc.r1p8 = !lbp_generic_forced() && r1p8_match(P, so, sw, oy, ox, by, bx, k);
    for (int i = 0; i < P; ++i) {
      sc.nterm[i] = g.nterm[i];
      for (int t = 0; t < 4; ++t) {
        sc.toff[i][t] = t < g.nterm[i] ? g.toff[i][t] : 0;
        sc.tw[i][t] = sc.r1p8 ? k.w[i][t] : (t < g.nterm[i] ? g.tw[i][t] : 0.0);
      }
    }
  }
  const int64_t row_bins = (int64_t)S * gr * gc * (1LL << P);
  if (row_bins > 0x7fffffffLL) return fail(OFR_E_UNSUPPORTED, who + ": feature row too long");
  if (rows) OFR_CHECK_ARG(ld >= row_bins && ld % 4 == 0, "ofr_mslbp_hist: ld must be a multiple of 4 that holds the row");
  // the fewest bands whose evened-out cell rows fit half the LDS (two workgroups per CU), else all of it
  const int plane_bytes = pixel_bytes == 1 ? 1 : 8;
  int64_t lds = 0;
  for (int64_t budget : {(int64_t)LDS_HALF, (int64_t)LDS_MAX}) {
    for (int nbands = 1; nbands <= gr && !a.nbands; ++nbands) {
      const int r = (int)cdiv(gr, nbands);
      lds = lds_bytes(a, r, plane_bytes);
      if (lds <= budget) {
        a.rows = r;
        a.nbands = (int)cdiv(gr, r);
      }
    }
    if (a.nbands) break;
  }
  if (!a.nbands) return fail(OFR_E_UNSUPPORTED, who + ": one cell row of all scales does not fit the LDS");
  if (n * a.nbands > 0x7fffffffLL) return fail(OFR_E_UNSUPPORTED, who + ": too many images");
  if (n == 0) return OFR_OK;
  OFR_CHECK_ARG(imgs, "ofr_mslbp_hist: null pointer");
  OFR_CHECK_ARG((uintptr_t)imgs % (uintptr_t)pixel_bytes == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)rows & 15) == 0,
                "ofr_mslbp_hist: images must be aligned to their pixels, counts to 4 bytes, rows to 16");
  hipStream_t st = (hipStream_t)stream;
  if (pixel_bytes == 1) return launch<uint8_t>(st, imgs, pixel_bytes, n, a, (size_t)lds, (uint32_t*)counts, rows);
  return launch<double>(st, imgs, pixel_bytes, n, a, (size_t)lds, (uint32_t*)counts, rows);
}
