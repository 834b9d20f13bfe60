// ExtendedLBP and OriginalLBP codes and per-cell histograms of float32 / float64 images on gfx950
// (bit-exact).  The float twins of ofr_lbp.hip and of the OriginalLBP half of ofr_lpq.hip: the faces the
// preprocessing kernels return (Tan-Triggs: float32 in (-tau, tau); equalisation: float64 in 0..255)
// go to the descriptors without a host trip.  LPQ's float path is the pixel-typed lpq_kernel of ofr_lpq.hip.
//
// Semantics (reference lbp.py:59-69, 80-130 on a float image, numpy 2.x): every pixel is converted
// exactly to fp64 and all arithmetic is fp64 without contraction.
//   OriginalLBP: eight >= compares of the ring against the centre value itself; bit 7..0 = NW, N, NE, E,
//                SE, S, SW, W.
//   ExtendedLBP: N = w1*X; N += w2*X; N += w3*X; N += w4*X (zero weights dropped on the host), bit i is
//                N >= C, and C is the reference's np.asarray(X, dtype=np.uint8) of the centre (lbp.py:104):
//                C = (double)((int64)trunc(x) & 255).  Here C = t - 256 floor(t / 256), t = trunc(x):
//                four exact fp64 operations, the same value for every |x| < 2^63, 0 beyond (every such
//                double is a multiple of 256; x86's out-of-range conversion also ends in 0), NaN for a
//                non-finite x.  A NaN compares false, so a code touching one only loses bits: nothing
//                traps and every code stays below 2^P.
//
// Design.  The byte kernels rest on 1-byte pixels (16 per staging load, image + counters inside 80 KiB,
// dword byte shuffles); none of that carries over.  Here the pixel width matters in ONE place:
//
// * Staging converts.  A workgroup (1024 threads) owns a band of cell rows of one image.  It stages the
//   band's pixel rows (py * rows + by - 1 of them, contiguous in memory) into LDS AS FP64, behind the u32
//   counters of the band's cells.  Each pixel is converted once per band, by the thread that loaded it;
//   from there on the kernels do not know the pixel type, every LDS read is one ds_read_b64 and feeds the
//   fp64 VALU directly.  Loads are 16 bytes (4 float32 / 2 float64) from the first 16-byte boundary of
//   the band on; the elements in front of it and behind the last whole vector go one by one.  That is
//   the rule for odd widths and odd band starts: alignment is a property of the band's first byte, not
//   of the row pitch, because the band's rows are contiguous.
// * Work split.  rows = cell rows per band is the largest whose counters + fp64 plane fit 80 KiB (two
//   workgroups per CU), else the largest that fits the 160 KiB of a gfx950 workgroup, then evened out
//   over the bands (8 cell rows that fit 3 at a time run as 3 + 3 + 2).  A 100 x 100 face at 8 x 8 cells
//   x 256 bins is two bands of 71 KiB; a 128 x 128 face three.  Bands of one image write disjoint
//   counters, so nothing meets in global memory.  14 x 12 cells are two bands.  When not even one
//   cell row fits (gc * 2^P counters above 160 KiB, or very wide images) the global form below runs:
//   pixels through L2, counters as packed atomics on a zeroed destination.
// * Lanes.  The band's code pixels are cut into `nstrips` strips of rows, nstrips = 1024 / width, and
//   thread i takes column i % width of strip i / width: adjacent lanes read adjacent fp64 values (unit
//   stride, conflict-free but where a wave wraps from one strip to the next), and a 98-column band keeps
//   980 of 1024 lanes busy where a fixed 128 x 8 split keeps 784.
// * Neighbour reuse, 3 x 3 forms (ExtendedLBP r = 1, P = 8 and OriginalLBP).  A thread walks its
//   column down the strip with the 3 x 3 block in 9 fp64 registers: per code pixel it reads the 3 values
//   of the new bottom row and shifts the block, instead of 21 (8) term reads.  The centre's C is
//   computed when the pixel sits at the block's centre, i.e. once per pixel; nothing is stored beside
//   the plane.  Per pixel that is 3 LDS reads, 21 multiplies + 13 adds + 8 compares + 4 for C.
// * Generic (radius, P <= 15).  Same staging, same lane map; per code pixel the points' terms are read
//   from the plane (offsets and weights are kernel arguments, scalar loads).  Not shaped further.
// * Counters leave LDS packed (4 / 2 / 1 per 32-bit store) as in the byte kernels.
#include "ofr_common.h"
#include "ofr_lbp_band.h"
#include "ofr_lbp_geom.h"

#pragma clang fp contract(off)

namespace ofr {
namespace lbpf {

enum { FORM_GENERIC = 0, FORM_R1P8 = 1, FORM_OLBP = 2 };

struct Band {
  int W;            // image row pitch = plane row pitch
  int img_rows;     // H
  int halo;         // by - 1: pixel rows below the last code row
  int gr, gc, py, px;
  int rows;         // cell rows per band
  int nbands;
  int nb_log2;
  int count_bytes;
  int pixel_bytes;
  int packed;       // 2^P * count_bytes is a multiple of 4: counts leave as whole 32-bit words
  int raw_centre;   // OriginalLBP: the centre value itself
  int coff;         // centre offset oy*W + ox
};

template <int FORM>
__global__ void __launch_bounds__(THREADS) band_hist_kernel(const void* __restrict__ imgs, LbpGeom g, Band a, R1P8 k,
                                                            void* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hist[];
  const int64_t img = blockIdx.x / a.nbands;
  const int band = blockIdx.x - (int)img * a.nbands;
  const int cr0 = band * a.rows, cr1 = min(a.gr, cr0 + a.rows);
  const int nb = 1 << a.nb_log2;
  const int total = (cr1 - cr0) * a.gc * nb;
  double* im = reinterpret_cast<double*>(hist + a.rows * a.gc * nb);  // 8-byte aligned: 2^P >= 2 counters per cell
  const int W = a.W;
  const int hpx = (cr1 - cr0) * a.py;  // code rows of the band
  const int wpx = a.gc * a.px;         // covered code columns
  for (int i = threadIdx.x; i < total; i += THREADS) hist[i] = 0;
  {
    const int64_t first = (img * a.img_rows + (int64_t)cr0 * a.py) * W;  // the band's first pixel
    const int count = (hpx + a.halo) * W;
    if (a.pixel_bytes == 4) stage_plane(reinterpret_cast<const float*>(imgs) + first, im, count);
    else stage_plane(reinterpret_cast<const double*>(imgs) + first, im, count);
  }
  __syncthreads();
  const int nstrips = max(1, min(hpx, THREADS / wpx));
  const int srows = (hpx + nstrips - 1) / nstrips;
  for (int item = threadIdx.x; item < nstrips * wpx; item += THREADS) {
    const int s = item / wpx, x = item - s * wpx;
    const int ya = s * srows, yb = min(hpx, ya + srows);
    if (ya >= yb) continue;
    const int cxo = x / a.px;
    int cyc = ya / a.py, ry = ya - cyc * a.py;
    const double* col = im + x;
    if constexpr (FORM == FORM_GENERIC) {
      for (int y = ya; y < yb; ++y) {
        const double* blk = col + y * W;
        const double c0 = blk[a.coff];
        const double C = a.raw_centre ? c0 : centre_u8(c0);
        uint32_t code = 0;
        for (int i = 0; i < g.P; ++i) {
          double N = g.tw[i][0] * blk[g.toff[i][0]];
          for (int t = 1; t < g.nterm[i]; ++t) {  // lbp.py:123-126 order, no contraction
            const double prod = g.tw[i][t] * blk[g.toff[i][t]];
            N = N + prod;
          }
          code |= (N >= C ? 1u : 0u) << i;
        }
        atomicAdd(&hist[(cyc * a.gc + cxo) * nb + (int)code], 1u);
        if (++ry == a.py) {
          ry = 0;
          ++cyc;
        }
      }
    } else {
      double b00 = col[ya * W], b01 = col[ya * W + 1], b02 = col[ya * W + 2];
      double b10 = col[(ya + 1) * W], b11 = col[(ya + 1) * W + 1], b12 = col[(ya + 1) * W + 2];
      for (int y = ya; y < yb; ++y) {
        const double* r2 = col + (y + 2) * W;
        const double b20 = r2[0], b21 = r2[1], b22 = r2[2];
        uint32_t code;
        if constexpr (FORM == FORM_OLBP) {
          const double C = b11;
          code = ((b00 >= C ? 1u : 0u) << 7) | ((b01 >= C ? 1u : 0u) << 6) | ((b02 >= C ? 1u : 0u) << 5) |
                 ((b12 >= C ? 1u : 0u) << 4) | ((b22 >= C ? 1u : 0u) << 3) | ((b21 >= C ? 1u : 0u) << 2) |
                 ((b20 >= C ? 1u : 0u) << 1) | (b10 >= C ? 1u : 0u);
        } else {
          const double C = centre_u8(b11);
          double N;
          code = 0;
          N = k.w[0][0] * b12;
          code |= (N >= C ? 1u : 0u) << 0;
          N = k.w[1][0] * b01; N = N + k.w[1][1] * b02; N = N + k.w[1][2] * b11; N = N + k.w[1][3] * b12;
          code |= (N >= C ? 1u : 0u) << 1;
          N = k.w[2][0] * b01;
          code |= (N >= C ? 1u : 0u) << 2;
          N = k.w[3][0] * b00; N = N + k.w[3][1] * b01; N = N + k.w[3][2] * b10; N = N + k.w[3][3] * b11;
          code |= (N >= C ? 1u : 0u) << 3;
          N = k.w[4][0] * b00; N = N + k.w[4][2] * b10;
          code |= (N >= C ? 1u : 0u) << 4;
          N = k.w[5][0] * b10; N = N + k.w[5][1] * b11; N = N + k.w[5][2] * b20; N = N + k.w[5][3] * b21;
          code |= (N >= C ? 1u : 0u) << 5;
          N = k.w[6][0] * b20; N = N + k.w[6][1] * b21;
          code |= (N >= C ? 1u : 0u) << 6;
          N = k.w[7][0] * b11; N = N + k.w[7][1] * b12; N = N + k.w[7][2] * b21; N = N + k.w[7][3] * b22;
          code |= (N >= C ? 1u : 0u) << 7;
        }
        atomicAdd(&hist[(cyc * a.gc + cxo) * nb + (int)code], 1u);
        if (++ry == a.py) {
          ry = 0;
          ++cyc;
        }
        b00 = b10; b01 = b11; b02 = b12;
        b10 = b20; b11 = b21; b12 = b22;
      }
    }
  }
  __syncthreads();
  const int64_t cell_base = img * (int64_t)a.gr * a.gc + (int64_t)cr0 * a.gc;
  flush_band(hist, total, counts, cell_base * nb, a.count_bytes, a.packed != 0);
}

// ---- global form: code images, and counts whose counters or pixel rows do not fit LDS ---------------
enum { OUT_CODES_U8 = 0, OUT_CODES_U32 = 1, OUT_COUNTS = 2 };

struct Global {
  int out;
  int gr, gc, py, px, nb_log2, count_bytes;
  int raw_centre, coff;
};

template <typename T>
__device__ __forceinline__ uint32_t code_global(const T* __restrict__ blk, const LbpGeom& g, const Global& a) {
  const double c0 = (double)blk[a.coff];
  const double C = a.raw_centre ? c0 : centre_u8(c0);
  uint32_t code = 0;
  for (int i = 0; i < g.P; ++i) {
    double N = g.tw[i][0] * (double)blk[g.toff[i][0]];
    for (int t = 1; t < g.nterm[i]; ++t) {
      const double prod = g.tw[i][t] * (double)blk[g.toff[i][t]];
      N = N + prod;
    }
    code |= (N >= C ? 1u : 0u) << i;
  }
  return code;
}

template <typename T>
__global__ void __launch_bounds__(256) global_kernel(const T* __restrict__ imgs, LbpGeom g, Global a,
                                                     void* __restrict__ out) {
  const int64_t img = blockIdx.y;
  const T* im = imgs + img * (int64_t)g.H * g.W;
  const int npx = g.dy * g.dx;
  const int nb = 1 << a.nb_log2;
  uint32_t* gcounts = reinterpret_cast<uint32_t*>((uint8_t*)out + img * (int64_t)a.gr * a.gc * nb * a.count_bytes);
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npx; p += gridDim.x * blockDim.x) {
    const int y = p / g.dx, x = p - y * g.dx;
    const uint32_t code = code_global(im + (int64_t)y * g.W + x, g, a);
    if (a.out == OUT_CODES_U8) {
      reinterpret_cast<uint8_t*>(out)[img * npx + p] = (uint8_t)code;
    } else if (a.out == OUT_CODES_U32) {
      reinterpret_cast<uint32_t*>(out)[img * npx + p] = code;
    } else if (y < a.gr * a.py && x < a.gc * a.px) {
      // counter idx of the image's packed destination: the word that holds it and its unit there (no
      // byte or half ever carries: a counter ends at most at the cell's pixel count)
      const int64_t idx = (int64_t)((y / a.py) * a.gc + x / a.px) * nb + code;
      if (a.count_bytes == 1) atomicAdd(gcounts + (idx >> 2), 1u << (8 * (int)(idx & 3)));
      else if (a.count_bytes == 2) atomicAdd(gcounts + (idx >> 1), 1u << (16 * (int)(idx & 1)));
      else atomicAdd(gcounts + idx, 1u);
    }
  }
}

__global__ void __launch_bounds__(256) zero_kernel(uint32_t* __restrict__ p, int64_t nwords) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nwords; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = 0;
}

// ---- host side ----------------------------------------------------------------------------------------
// OriginalLBP as a geometry: eight single-term points of weight 1 (1.0 * x = x exactly), bit 7..0 = NW, N,
// NE, E, SE, S, SW, W
static void olbp_geom(LbpGeom& g, int H, int W) {
  static const int ring[8][2] = {{1, 0}, {2, 0}, {2, 1}, {2, 2}, {1, 2}, {0, 2}, {0, 1}, {0, 0}};  // bit 0..7
  g.P = 8;
  g.H = H;
  g.W = W;
  g.dy = H - 2;
  g.dx = W - 2;
  g.oy = g.ox = 1;
  for (int i = 0; i < 8; ++i) {
    g.nterm[i] = 1;
    g.toff[i][0] = ring[i][0] * W + ring[i][1];
    g.tw[i][0] = 1.0;
  }
}

static int launch_global(hipStream_t st, const void* imgs, int pixel_bytes, int64_t n, const LbpGeom& g,
                         const Global& a, void* out, size_t img_out_bytes) {
  const int npx = g.dy * g.dx;
  const unsigned gx = (unsigned)std::min<int64_t>(cdiv(npx, 256), 64);
  const int64_t img_px = (int64_t)g.H * g.W;
  for (int64_t done = 0; done < n; done += 65535) {
    const int64_t chunk = std::min<int64_t>(n - done, 65535);
    void* o = (void*)((char*)out + done * (int64_t)img_out_bytes);
    if (pixel_bytes == 4)
      hipLaunchKernelGGL(global_kernel<float>, dim3(gx, (unsigned)chunk), dim3(256), 0, st,
                         (const float*)imgs + done * img_px, g, a, o);
    else
      hipLaunchKernelGGL(global_kernel<double>, dim3(gx, (unsigned)chunk), dim3(256), 0, st,
                         (const double*)imgs + done * img_px, g, a, o);
    OFR_LAUNCH_CHECK("lbp float global_kernel");
  }
  return OFR_OK;
}

static int check_centre(const std::string& w, int oy, int ox, int by, int bx) {
  if (oy < 0 || ox < 0 || oy >= by || ox >= bx) return fail(OFR_E_INVALID, w + ": centre outside the block");
  return OFR_OK;
}

static int check_common(const std::string& w, const void* imgs, int pixel_bytes, int64_t n, int H, int W) {
  if (n < 0 || H < 1 || W < 1) return fail(OFR_E_INVALID, w + ": bad sizes");
  if (pixel_bytes != 4 && pixel_bytes != 8) return fail(OFR_E_INVALID, w + ": pixel_bytes must be 4 (float32) or 8 (float64)");
  if ((int64_t)H * W > 0x7fffffffLL / 2) return fail(OFR_E_UNSUPPORTED, w + ": image too large");
  if ((uintptr_t)imgs % (uintptr_t)pixel_bytes) return fail(OFR_E_INVALID, w + ": images must be aligned to their pixels");
  return OFR_OK;
}

static int run_codes(const char* who, void* stream, const void* imgs, int pixel_bytes, int64_t n, const LbpGeom& g,
                     bool olbp, void* codes) {
  if (n == 0 || g.dy <= 0 || g.dx <= 0) return OFR_OK;
  if (!imgs || !codes) return fail(OFR_E_INVALID, std::string(who) + ": null pointer");
  Global a = {};
  a.out = olbp ? OUT_CODES_U8 : OUT_CODES_U32;
  a.gr = a.gc = a.py = a.px = 1;
  a.count_bytes = 1;
  a.raw_centre = olbp ? 1 : 0;
  a.coff = g.oy * g.W + g.ox;
  return launch_global((hipStream_t)stream, imgs, pixel_bytes, n, g, a, codes,
                       (size_t)g.dy * g.dx * (olbp ? 1 : 4));
}

template <int FORM>
static int launch_band(hipStream_t st, const void* imgs, int64_t n, const LbpGeom& g, const Band& a, const R1P8& k,
                       size_t lds, void* counts) {
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute((const void*)band_hist_kernel<FORM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       LDS_MAX);
    if (e != hipSuccess) return hip_status(e, "hipFuncSetAttribute(lbp float band_hist_kernel)");
    attr = true;
  }
  hipLaunchKernelGGL(band_hist_kernel<FORM>, dim3((unsigned)(n * a.nbands)), dim3(THREADS), lds, st, imgs, g, a, k,
                     counts);
  OFR_LAUNCH_CHECK("lbp float band_hist_kernel");
  return OFR_OK;
}

// g, by (block rows) and the grid are checked; py * px > 0
static int run_hist(const char* who, void* stream, const void* imgs, int pixel_bytes, int64_t n, const LbpGeom& g,
                    int by, int form, const R1P8& k, int gr, int gc, int py, int px, void* counts, int count_bytes) {
  const std::string w(who);
  const int P = g.P;
  const int64_t nb = 1LL << P;
  const int64_t img_counts = (int64_t)gr * gc * nb * count_bytes;
  if (n == 0) return OFR_OK;
  if (!imgs || !counts) return fail(OFR_E_INVALID, w + ": null pointer");
  if ((uintptr_t)counts & 3) return fail(OFR_E_INVALID, w + ": counts must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  // cell rows per band: counters + fp64 plane of the band's pixel rows
  const int64_t row_cnt = (int64_t)gc * nb * 4, row_px = (int64_t)py * g.W * 8, halo_px = (int64_t)(by - 1) * g.W * 8;
  auto fit = [&](int64_t budget) { return std::min<int64_t>(gr, (budget - halo_px) / (row_cnt + row_px)); };
  int64_t rows = fit(LDS_HALF);
  if (rows < 1) rows = fit(LDS_MAX);
  if (rows >= 1 && n * cdiv(gr, rows) <= 0x7fffffffLL) {
    Band a = {};
    a.W = g.W;
    a.img_rows = g.H;
    a.halo = by - 1;
    a.gr = gr;
    a.gc = gc;
    a.py = py;
    a.px = px;
    a.nbands = (int)cdiv(gr, rows);
    a.rows = (int)cdiv(gr, a.nbands);
    a.nb_log2 = P;
    a.count_bytes = count_bytes;
    a.pixel_bytes = pixel_bytes;
    a.packed = (nb * count_bytes) % 4 == 0;
    a.raw_centre = form == FORM_OLBP;
    a.coff = g.oy * g.W + g.ox;
    const size_t lds = (size_t)(a.rows * (row_cnt + row_px) + halo_px);
    if (form == FORM_R1P8) return launch_band<FORM_R1P8>(st, imgs, n, g, a, k, lds, counts);
    if (form == FORM_OLBP) return launch_band<FORM_OLBP>(st, imgs, n, g, a, k, lds, counts);
    return launch_band<FORM_GENERIC>(st, imgs, n, g, a, k, lds, counts);
  }
  // global form: packed atomics need each image's counts to fill whole words
  if (img_counts % 4) return fail(OFR_E_UNSUPPORTED, w + ": counts of one image must fill whole 32-bit words here");
  const int64_t nwords = n * (img_counts / 4);
  hipLaunchKernelGGL(zero_kernel, dim3((unsigned)std::min<int64_t>(cdiv(nwords, 256), 4096)), dim3(256), 0, st,
                     (uint32_t*)counts, nwords);
  OFR_LAUNCH_CHECK("lbp float zero_kernel");
  Global a = {};
  a.out = OUT_COUNTS;
  a.gr = gr;
  a.gc = gc;
  a.py = py;
  a.px = px;
  a.nb_log2 = P;
  a.count_bytes = count_bytes;
  a.raw_centre = form == FORM_OLBP;
  a.coff = g.oy * g.W + g.ox;
  return launch_global(st, imgs, pixel_bytes, n, g, a, counts, (size_t)img_counts);
}

}  // namespace lbpf
}  // namespace ofr

using namespace ofr;
using namespace ofr::lbpf;

extern "C" int ofr_elbp_codes_f(void* stream, const void* imgs, int pixel_bytes, int64_t n, int H, int W, int P,
                                const int32_t* offs_host, const double* w_host, int oy, int ox, int by, int bx,
                                uint32_t* codes) {
  int rc = check_common("ofr_elbp_codes_f", imgs, pixel_bytes, n, H, W);
  if (rc) return rc;
  LbpGeom g;
  rc = make_geom(g, H, W, P, offs_host, w_host, oy, ox, by, bx);
  if (rc) return rc;
  rc = check_centre("ofr_elbp_f", oy, ox, by, bx);
  if (rc) return rc;
  return run_codes("ofr_elbp_codes_f", stream, imgs, pixel_bytes, n, g, false, codes);
}

extern "C" int ofr_elbp_hist_f(void* stream, const void* imgs, int pixel_bytes, int64_t n, int H, int W, int P,
                               const int32_t* offs_host, const double* w_host, int oy, int ox, int by, int bx, int gr,
                               int gc, void* counts, int count_bytes) {
  int rc = check_common("ofr_elbp_hist_f", imgs, pixel_bytes, n, H, W);
  if (rc) return rc;
  OFR_CHECK_ARG(gr >= 1 && gc >= 1, "ofr_elbp_hist_f: bad grid");
  OFR_CHECK_ARG(count_bytes == 1 || count_bytes == 2 || count_bytes == 4, "ofr_elbp_hist_f: count_bytes must be 1, 2 or 4");
  if (P > 15) return fail(OFR_E_UNSUPPORTED, "ofr_elbp_hist_f: neighbors must be <= 15 for the histogram");
  LbpGeom g;
  rc = make_geom(g, H, W, P, offs_host, w_host, oy, ox, by, bx);
  if (rc) return rc;
  rc = check_centre("ofr_elbp_f", oy, ox, by, bx);
  if (rc) return rc;
  const int py = g.dy > 0 ? g.dy / gr : 0, px = g.dx > 0 ? g.dx / gc : 0;
  const int64_t cell_px = (int64_t)py * px;
  if (count_bytes == 1) OFR_CHECK_ARG(cell_px <= 255, "ofr_elbp_hist_f: cell too large for 1-byte counts");
  if (count_bytes == 2) OFR_CHECK_ARG(cell_px <= 65535, "ofr_elbp_hist_f: cell too large for 2-byte counts");
  if (n == 0) return OFR_OK;
  if (cell_px == 0) {  // empty cells: all counts zero (the reference's histogram is then NaN)
    OFR_CHECK_ARG(counts, "ofr_elbp_hist_f: null pointer");
    const int64_t nbytes = n * gr * gc * (1LL << P) * count_bytes;
    OFR_CHECK_ARG(((uintptr_t)counts & 3) == 0 && nbytes % 4 == 0, "ofr_elbp_hist_f: counts must be whole 32-bit words");
    hipLaunchKernelGGL(zero_kernel, dim3((unsigned)std::min<int64_t>(cdiv(nbytes / 4, 256), 4096)), dim3(256), 0,
                       (hipStream_t)stream, (uint32_t*)counts, nbytes / 4);
    OFR_LAUNCH_CHECK("lbp float zero_kernel");
    return OFR_OK;
  }
  R1P8 k = {};
  const bool r1p8 = !lbp_generic_forced() && r1p8_match(P, offs_host, w_host, oy, ox, by, bx, k);
  return run_hist("ofr_elbp_hist_f", stream, imgs, pixel_bytes, n, g, by, r1p8 ? FORM_R1P8 : FORM_GENERIC, k, gr, gc,
                  py, px, counts, count_bytes);
}

extern "C" int ofr_olbp_codes_f(void* stream, const void* imgs, int pixel_bytes, int64_t n, int H, int W,
                                uint8_t* codes) {
  int rc = check_common("ofr_olbp_codes_f", imgs, pixel_bytes, n, H, W);
  if (rc) return rc;
  LbpGeom g;
  olbp_geom(g, H, W);
  return run_codes("ofr_olbp_codes_f", stream, imgs, pixel_bytes, n, g, true, codes);
}

extern "C" int ofr_olbp_hist_f(void* stream, const void* imgs, int pixel_bytes, int64_t n, int H, int W, int gr,
                               int gc, void* counts, int count_bytes) {
  int rc = check_common("ofr_olbp_hist_f", imgs, pixel_bytes, n, H, W);
  if (rc) return rc;
  LbpGeom g;
  olbp_geom(g, H, W);
  OFR_CHECK_ARG(gr >= 1 && gc >= 1, "ofr_olbp_hist_f: bad grid");
  OFR_CHECK_ARG(count_bytes == 1 || count_bytes == 2 || count_bytes == 4, "ofr_olbp_hist_f: count_bytes must be 1, 2 or 4");
  OFR_CHECK_ARG(gr <= g.dy && gc <= g.dx, "ofr_olbp_hist_f: grid larger than the code image");
  const int py = g.dy / gr, px = g.dx / gc;
  const int64_t cell_px = (int64_t)py * px;
  OFR_CHECK_ARG(!(count_bytes == 1 && cell_px > 255) && !(count_bytes == 2 && cell_px > 65535),
                "ofr_olbp_hist_f: cell too large for count_bytes");
  R1P8 k = {};
  return run_hist("ofr_olbp_hist_f", stream, imgs, pixel_bytes, n, g, 3, lbp_generic_forced() ? FORM_GENERIC : FORM_OLBP,
                  k, gr, gc, py, px, counts, count_bytes);
}
