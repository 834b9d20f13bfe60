// NormalizedCorrelation nearest-neighbour search on gfx950.
//
// Replaces NormalizedCorrelation (reference distance.py:80-98) inside NearestNeighbor.predict
// (classifier.py:104-119):
//     d(p, q) = 1 - (p - pm).(q - qm) / (|p - pm| |q - qm|),   pm, qm the row means.
// d lies in [0, 2], is invariant under p -> s p + t (s > 0) -- so counts need no denominator -- and is
// bilinear in the centred rows: the one LBPH metric that fits a matrix instruction without a table.
//
//   ncc_stats_kernel   per row (mean, 1 / |x - mean|), one wave per row.  uint8 / uint16 counts: the exact
//                      integers S = sum x and V = n sum x^2 - S^2 (64-bit, 128-bit loads + v_sad_u8 /
//                      v_dot4_u32_u8 for uint8), |x - mean|^2 = V / n rounded once.  uint32 / fp32 rows (and
//                      uint16 rows too long for the 64-bit V): two fp64 passes, mean then sum (x - mean)^2.
//   ncc_mfma_kernel    coarse pass of uint8 counts on v_mfma_i32_32x32x32_i8.  Operands a' = a - 128 (XOR 0x80
//                      on the fragments), so with L the padded row length
//                          sum a c = sum a' c' + 128 (Sa + Sc) - 2^14 L            (exact, 64-bit)
//                          num     = n sum a c - Sq Sg                              (exact, 64-bit)
//                          score   = 1 - (num / n) rq rg                            (fp64, rounded once to fp32).
//                      Tile design.  The shared engine of ofr_i8_tile.h was NOT reused: its LDS-DMA copies whole
//                      128-byte lines and clamps columns past the row back into it, which needs ld % 128 == 0
//                      and pad bytes of 128 (ofr_gram_u8's contract).  LBPH rows are ld = round_up(nbins, 16)
//                      with zero pads, and a query batch straight from SpatialHistogram has no pad at all.  So
//                      this kernel stages through registers, where the tail can be masked: a workgroup of 4
//                      waves owns 128 gallery x 128 query rows, each wave 64 x 64 (2 x 2 MFMA blocks, 64
//                      accumulator registers); a k step is 128 bytes of every row, 16 KiB per operand in LDS
//                      (the engine's XOR-swizzled 128-byte rows, conflict-free ds_read_b128 fragments); each
//                      thread carries 4 + 4 128-bit global loads of the NEXT step while the 16 MFMAs of the
//                      current one run (one LDS buffer, two barriers per step).  Bytes at or past nbins are
//                      zeroed in registers, whatever the pad holds; chunks past the row are not read.  Both
//                      operands then hold -128 there, which is the 2^14 L term above with L = 128 ceil(nbins / 128).
//                      The int32 accumulator bounds one chain to L 2^14 < 2^31: rows of 2^17 bytes or more take
//                      the general kernel instead (no k chunking here).
//   ncc_tile_kernel    every other case (uint16 / uint32 / fp32 rows, long uint8 rows): hist_tile_kernel's
//                      shape, 64 x 64 pairs per workgroup, 4 x 4 per thread, 64 bins per stage.  Values are
//                      widened and centred by their row mean (fp64 subtract, one fp32 rounding) on the LDS
//                      write, so the epilogue has no n mq mg cancellation; the dot product is a scalar fp32 FMA
//                      chain per pair.  A tile that meets a uint32 count >= 2^24 gets the key -inf for every pair:
//                      its rows stay candidates and none of its queries is certified.
//   ncc_rerank_kernel  per query the best 16 over all tile lists, each re-evaluated by the reference formula in
//                      fp64 (means, centred dot, two square roots, 1 - quotient), sorted by (distance, row) with
//                      NaN last, and the certificate.
//
// Keys.  A zero-variance row has 1 / |x - mean| = inf and the reference distance 0 / 0 = NaN: its key is +inf
// (so is every key of a zero-variance query, which is never certified).  NaN scores become +inf as well.
//
// Certificate (absolute: d is in [0, 2] and exactly 0 for proportional rows, so no relative rule applies).
// Let e be a bound on |key - d| over all pairs, d the fp64 reference value the re-rank computes.  Every row
// outside the 16 candidates has key >= tau (the 16th candidate's key), hence d >= tau - e; the top-k is exact
// iff the k-th exact distance lies strictly below tau - e.  u = 2^-24:
//   * key rounding: the score is formed in fp64 and rounded once to fp32; |score| <= 2 (+ e), so <= 2 u;
//   * MFMA pass: num is an exact integer below 2^53; rq, rg carry a few fp64 roundings: < 2^-40 with room;
//   * general pass: a staged value is fl(x - mean) = (x - mean)(1 + d1), |d1| <= u; a product of two such,
//     accumulated by n sequential FMAs, errs by <= ((1 + u)^(n + 2) - 1) sum |p_i q_i|, and
//     sum |p_i q_i| <= |p - pm| |q - qm| (Cauchy-Schwarz), which the factor rq rg cancels: <= 1.0625 (n + 2) u
//     while n u < 1/16 (beyond that the bound is useless anyway and nothing certifies);
//   * the re-rank's own fp64 sums: (nbins + 16) 2^-50 with room.
// e = 2 u + 2^-40 + (nbins + 16) 2^-50   [+ 1.0625 (nbins + 2) u for the general kernel].
//
// The fp32 sums are scalar: the file is built with the packed-fp32 target feature off (see the Makefile rule).
#include <cmath>

#include "ofr_i8_tile.h"
#include "ofr_keys.h"
#include "ofr_topk.h"

namespace ofr {
namespace ncc {

enum { DT_U8 = OFR_DT_U8, DT_U16 = OFR_DT_U16, DT_U32 = OFR_DT_U32, DT_F32 = OFR_DT_F32 };
constexpr int KC = keys::KC;      // candidates per (query, tile)
constexpr int TT = 64, BB = 64;   // general kernel: rows per tile side, bins per stage
constexpr int SP = TT + 1;        // pitch of its score tile in LDS
constexpr int MT = 128, BK = 128; // MFMA kernel: rows per tile side, bytes of a row per k step
constexpr int PANEL = MT * BK;    // 16 KiB per operand

template <int DT> struct Elem { typedef float T; };
template <> struct Elem<DT_U8> { typedef uint8_t T; };
template <> struct Elem<DT_U16> { typedef uint16_t T; };
template <> struct Elem<DT_U32> { typedef uint32_t T; };

struct RowStat {
  double mean;     // sum x / n
  double rinv;     // 1 / |x - mean| (inf for a constant row)
  long long sum;   // sum x, exact (integer path; 0 otherwise)
  long long wide;  // uint32 rows: a count >= 2^24 was seen
};

template <int DT>
__device__ __forceinline__ double load1(const void* base, int64_t idx) {
  return (double)reinterpret_cast<const typename Elem<DT>::T*>(base)[idx];
}

// 16 consecutive values of a 16-byte aligned row as fp32 (128-bit loads)
template <int DT>
__device__ __forceinline__ void load16(const void* base, int64_t idx, float (&v)[16]) {
  typedef typename Elem<DT>::T T;
  constexpr int PER = 16 / (int)sizeof(T);
  const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(base) + idx);
#pragma unroll
  for (int h = 0; h < 16 / PER; ++h) {
    const uint4 x = src[h];
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if constexpr (DT == DT_U8) v[h * PER + i] = (float)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
      else if constexpr (DT == DT_U16) v[h * PER + i] = (float)((w[i >> 1] >> (16 * (i & 1))) & 0xffffu);
      else if constexpr (DT == DT_U32) v[h * PER + i] = (float)w[i];
      else v[h * PER + i] = __uint_as_float(w[i]);
    }
  }
}

// the 16 bytes at `off` of a uint8 row of nb bins; bytes at or past nb read as 0, a chunk that starts there is
// not read at all (rows are 16-byte aligned with ld >= nb, ld % 16 == 0: a chunk that starts below nb lies
// inside the row)
__device__ __forceinline__ uint4 load_u8x16(const uint8_t* row, int64_t off, int64_t nb) {
  uint4 x = make_uint4(0u, 0u, 0u, 0u);
  if (off < nb) {
    x = *reinterpret_cast<const uint4*>(row + off);
    const int64_t rem = nb - off;   // > 0
    if (rem < 16) {
      uint32_t v[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = (int)rem - 4 * j;
        v[j] = r >= 4 ? v[j] : r <= 0 ? 0u : (v[j] & ((1u << (8 * r)) - 1u));
      }
      x = make_uint4(v[0], v[1], v[2], v[3]);
    }
  }
  return x;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o);
  return v;
}

// ---- row statistics ---------------------------------------------------------------------------------------
// INTEGER: the exact 64-bit path (uint8 / uint16 with nbins^2 max^2 < 2^63, checked on the host)
template <int DT, bool INTEGER>
__global__ void __launch_bounds__(256) ncc_stats_kernel(const void* X, int64_t rows, int64_t ld, int64_t nbins,
                                                        RowStat* out) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // one wave per row
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  const double n = (double)nbins;
  RowStat s;
  if constexpr (INTEGER) {
    unsigned long long S = 0, SS = 0;
    if constexpr (DT == DT_U8) {
      const uint8_t* x = reinterpret_cast<const uint8_t*>(X) + r * ld;
      for (int64_t b = (int64_t)lane * 16; b < nbins; b += 64 * 16) {
        const uint4 v = load_u8x16(x, b, nbins);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          S += __builtin_amdgcn_sad_u8(w[j], 0u, 0u);
          SS += __builtin_amdgcn_udot4(w[j], w[j], 0u, false);
        }
      }
    } else {
      const uint16_t* x = reinterpret_cast<const uint16_t*>(X) + r * ld;
      for (int64_t b = lane; b < nbins; b += 64) {
        const unsigned long long v = x[b];
        S += v;
        SS += v * v;
      }
    }
    S = wave_sum(S);
    SS = wave_sum(SS);
    const unsigned long long V = (unsigned long long)nbins * SS - S * S;   // >= 0 (Cauchy-Schwarz), exact
    s.mean = (double)S / n;
    s.rinv = sqrt(n / (double)V);   // |x - mean|^2 = V / n; V = 0 -> inf
    s.sum = (long long)S;
    s.wide = 0;
  } else {
    double a = 0;
    bool wide = false;
    for (int64_t b = lane; b < nbins; b += 64) {
      const double v = load1<DT>(X, r * ld + b);
      a += v;
      if constexpr (DT == DT_U32) wide |= v >= 16777216.0;
    }
    const double mean = wave_sum(a) / n;
    double c = 0;
    for (int64_t b = lane; b < nbins; b += 64) {
      const double d = load1<DT>(X, r * ld + b) - mean;
      c = fma(d, d, c);
    }
    c = wave_sum(c);
    s.mean = mean;
    s.rinv = 1.0 / sqrt(c);
    s.sum = 0;
    s.wide = __ballot(wide) != 0;
  }
  if (lane == 0) out[r] = s;
}

// score of a pair -> fp32 key (+inf for a zero-variance row and for NaN)
__device__ __forceinline__ float score_key(double corr, double rq, double rg) {
  const double s = 1.0 - corr * rq * rg;
  return (rq < __builtin_inf() && rg < __builtin_inf() && s == s) ? (float)s : __builtin_inff();
}

struct Args {
  const void* Q;
  int64_t B, ldq;
  const void* G;
  int64_t N, ldg, nbins;
  const RowStat* sq;   // [B]
  const RowStat* sg;   // [N]
  Cand* cand;          // [ntg][B][KC]
  int64_t ntq, ntg;
};

// ---- (a) uint8 counts on the int8 MFMA ---------------------------------------------------------------------
__global__ void __launch_bounds__(256) ncc_mfma_kernel(Args p) {
  using i8t::i32x16;
  using i8t::i32x4;
  __shared__ __attribute__((aligned(16))) char smem[2 * PANEL];   // gallery panel, query panel; then the lists
  __shared__ long long sum_g[MT], sum_q[MT];
  __shared__ double rinv_g[MT], rinv_q[MT];
  const int64_t t = blockIdx.x;
  const int64_t gt = t / p.ntq, qt = t % p.ntq;   // consecutive blocks share the gallery tile
  const int64_t g0 = gt * MT, q0 = qt * MT;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wr = wave >> 1, wc = wave & 1, h = lane >> 5, r32 = lane & 31;
  // staging: thread -> 16-byte chunk (tid & 7) of rows (tid >> 3) + 32 j; 8 lanes cover one row's 128 bytes
  const int lchunk = tid & 7, lrow = tid >> 3;
  const uint8_t* grow[4];
  const uint8_t* qrow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    grow[j] = reinterpret_cast<const uint8_t*>(p.G) + min(g0 + lrow + 32 * j, p.N - 1) * p.ldg;
    qrow[j] = reinterpret_cast<const uint8_t*>(p.Q) + min(q0 + lrow + 32 * j, p.B - 1) * p.ldq;
  }
  i32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

  uint4 wg[4], wq[4];
  auto fetch = [&](int kt) {
    const int64_t off = (int64_t)kt * BK + lchunk * 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      wg[j] = load_u8x16(grow[j], off, p.nbins);
      wq[j] = load_u8x16(qrow[j], off, p.nbins);
    }
  };
  const int nk = (int)cdiv(p.nbins, BK);
  fetch(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();   // every wave is done with the previous step's fragments
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *reinterpret_cast<uint4*>(smem + i8t::off(lrow + 32 * j, lchunk)) = wg[j];
      *reinterpret_cast<uint4*>(smem + PANEL + i8t::off(lrow + 32 * j, lchunk)) = wq[j];
    }
    __syncthreads();
    if (kt + 1 < nk) fetch(kt + 1);   // in flight during this step's MFMAs
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      const int c = 2 * ks + h;   // lanes 0-31: k bytes 0-15 of the MFMA's 32, lanes 32-63: 16-31
      i32x4 gf[2], qf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        gf[i] = *reinterpret_cast<const i32x4*>(smem + i8t::off(wr * 64 + i * 32 + r32, c));
        gf[i] ^= (int)0x80808080;   // uint8 x -> int8 x - 128
        qf[i] = *reinterpret_cast<const i32x4*>(smem + PANEL + i8t::off(wc * 64 + i * 32 + r32, c));
        qf[i] ^= (int)0x80808080;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(gf[i], qf[j], acc[i][j], 0, 0, 0);
    }
  }
  __syncthreads();
  if (tid < MT) {
    const RowStat s = p.sg[min(g0 + tid, p.N - 1)];
    sum_g[tid] = s.sum;
    rinv_g[tid] = s.rinv;
  } else {
    const RowStat s = p.sq[min(q0 + tid - MT, p.B - 1)];
    sum_q[tid - MT] = s.sum;
    rinv_q[tid - MT] = s.rinv;
  }
  __syncthreads();
  // epilogue.  C/D of v_mfma_i32_32x32x32_i8: column (query) = lane & 31, row (gallery) = (reg & 3) +
  // 8 (reg >> 2) + 4 (lane >> 5).  A lane keeps the best KC of its 32 rows per query, merges with the other
  // half-wave (shuffles), then the two row-waves merge through LDS.
  Cand* kbuf = reinterpret_cast<Cand*>(smem);   // [2][MT][KC] = 32 KiB
  const long long n = p.nbins, lpad = (long long)nk * BK;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int ql = wc * 64 + j * 32 + r32;
    const long long sq = sum_q[ql];
    const double rq = rinv_q[ql];
    TopList<KC> L;
    L.init();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gl = wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const long long sg = sum_g[gl];
        const long long dot = (long long)acc[i][j][r] + 128 * (sq + sg) - 16384 * lpad;
        const long long num = n * dot - sq * sg;
        // the centred dot product is num / n (one fp64 rounding)
        if (g0 + gl < p.N) L.insert(score_key((double)num / (double)n, rq, rinv_g[gl]), (int)(g0 + gl));
      }
    float od[KC];
    int oi[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      od[c] = __shfl_xor(L.d[c], 32);
      oi[c] = __shfl_xor(L.i[c], 32);
    }
    L.merge(od, oi);
    if (h == 0) {
#pragma unroll
      for (int c = 0; c < KC; ++c) kbuf[((size_t)wr * MT + ql) * KC + c] = Cand{L.d[c], L.i[c]};
    }
  }
  __syncthreads();
  if (tid < MT) {
    TopList<KC> L;
    float od[KC];
    int oi[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const Cand x = kbuf[(size_t)tid * KC + c], y = kbuf[((size_t)MT + tid) * KC + c];
      L.d[c] = x.d;
      L.i[c] = x.i;
      od[c] = y.d;
      oi[c] = y.i;
    }
    L.merge(od, oi);
    if (q0 + tid < p.B) {
      Cand* out = p.cand + ((size_t)gt * p.B + q0 + tid) * KC;
#pragma unroll
      for (int c = 0; c < KC; ++c) out[c] = Cand{L.d[c], L.i[c]};
    }
  }
}

// ---- (b) every other element type: centred fp32 values, scalar fp32 FMA dot ---------------------------------
template <int DT>
__global__ void __launch_bounds__(256) ncc_tile_kernel(Args p) {
  __shared__ __attribute__((aligned(16))) float Qs[BB * TT];   // [bin][row]
  __shared__ __attribute__((aligned(16))) float Gs[BB * TT];
  __shared__ float S[TT * SP];
  const int64_t t = blockIdx.x;
  const int64_t gt = t / p.ntq, qt = t % p.ntq;
  const int64_t q0 = qt * TT, g0 = gt * TT;
  const int tid = threadIdx.x;
  const int tq = tid >> 4, tg = tid & 15;       // compute: queries tq*4.., gallery tg*4..
  const int lrow = tid >> 2, lseg = tid & 3;    // staging: row, 16-bin segment
  const int64_t qrow = min(q0 + lrow, p.B - 1), grow = min(g0 + lrow, p.N - 1);
  const double mq = p.sq[qrow].mean, mg = p.sg[grow].mean;

  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  bool wide = false;   // uint32 counts >= 2^24 are rounded on the way to fp32: the tile certifies nothing
  if constexpr (DT == DT_U32) wide = p.sq[qrow].wide != 0 || p.sg[grow].wide != 0;
  float vq[16], vg[16];
  const int nsteps = (int)(p.nbins / BB);
  if (nsteps > 0) {
    load16<DT>(p.Q, qrow * p.ldq + lseg * 16, vq);
    load16<DT>(p.G, grow * p.ldg + lseg * 16, vg);
  }
  for (int s = 0; s < nsteps; ++s) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      Qs[(lseg * 16 + i) * TT + lrow] = (float)((double)vq[i] - mq);
      Gs[(lseg * 16 + i) * TT + lrow] = (float)((double)vg[i] - mg);
    }
    __syncthreads();
    if (s + 1 < nsteps) {
      load16<DT>(p.Q, qrow * p.ldq + (int64_t)(s + 1) * BB + lseg * 16, vq);
      load16<DT>(p.G, grow * p.ldg + (int64_t)(s + 1) * BB + lseg * 16, vg);
    }
#pragma unroll 4
    for (int b = 0; b < BB; ++b) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&Qs[b * TT + tq * 4]);
      const f32x4 c = *reinterpret_cast<const f32x4*>(&Gs[b * TT + tg * 4]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(a[i], c[j], acc[i][j]);
    }
  }
  // this thread's own rows: means for the tail, 1 / norm for the epilogue
  double rq[4], rg[4], mqc[4], mgc[4];
  int64_t qr[4], gr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    qr[i] = min(q0 + tq * 4 + i, p.B - 1);
    gr[i] = min(g0 + tg * 4 + i, p.N - 1);
    const RowStat a = p.sq[qr[i]], c = p.sg[gr[i]];
    rq[i] = a.rinv;
    mqc[i] = a.mean;
    rg[i] = c.rinv;
    mgc[i] = c.mean;
  }
  // tail bins (nbins % 64): plain loads
  for (int64_t b = (int64_t)nsteps * BB; b < p.nbins; ++b) {
    float a[4], c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = (float)((double)(float)load1<DT>(p.Q, qr[i] * p.ldq + b) - mqc[i]);
      c[i] = (float)((double)(float)load1<DT>(p.G, gr[i] * p.ldg + b) - mgc[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(a[i], c[j], acc[i][j]);
  }
  if constexpr (DT == DT_U32) wide = __syncthreads_or(wide);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      S[(tq * 4 + i) * SP + tg * 4 + j] = wide ? -__builtin_inff() : score_key((double)acc[i][j], rq[i], rg[j]);
  __syncthreads();
  if (tid < TT) {
    TopList<KC> L;
    L.init();
    for (int j = 0; j < TT; ++j) {
      const int64_t g = g0 + j;
      if (g < p.N) L.insert(S[tid * SP + j], (int)g);
    }
    if (q0 + tid < p.B) {
      Cand* out = p.cand + ((size_t)gt * p.B + q0 + tid) * KC;
#pragma unroll
      for (int j = 0; j < KC; ++j) out[j] = Cand{L.d[j], L.i[j]};
    }
  }
}

// ---- (c) fp64 re-rank and certificate -----------------------------------------------------------------------
struct RerankArgs {
  const Cand* cand;
  int64_t T, B;
  const void* Q;
  int64_t ldq;
  const void* G;
  int64_t ldg, nbins;
  int k;
  int64_t index_base;
  double* out_d;
  int64_t* out_i;
  int* cert;      // nullable: 1 iff the result is provably the exact fp64 top-k
  double bound;   // |coarse key - exact distance| <= bound (file header)
};

template <int DT>
__global__ void __launch_bounds__(256) ncc_rerank_kernel(RerankArgs p) {
  __shared__ Cand lists[256 * KC];
  __shared__ double exact[KC];
  __shared__ double red[4];
  const int64_t q = blockIdx.x;
  select_candidates<KC>(p.cand, p.T, p.B, q, lists);
  const double n = (double)p.nbins;
  // distance.py:92-98 with p the gallery row, q the query: means, centred rows, 1 - pm.qm / (|pm| |qm|)
  double a = 0;
  for (int64_t b = threadIdx.x; b < p.nbins; b += blockDim.x) a += load1<DT>(p.Q, q * p.ldq + b);
  const double qmu = block_sum_f64(a, red) / n;
  a = 0;
  for (int64_t b = threadIdx.x; b < p.nbins; b += blockDim.x) {
    const double x = load1<DT>(p.Q, q * p.ldq + b) - qmu;
    a = fma(x, x, a);
  }
  const double qq = block_sum_f64(a, red);
  for (int c = 0; c < KC; ++c) {
    const Cand cc = lists[c];
    double val = __builtin_inf();
    if (cc.i != CAND_EMPTY) {
      const int64_t g = (int64_t)cc.i * p.ldg;
      a = 0;
      for (int64_t b = threadIdx.x; b < p.nbins; b += blockDim.x) a += load1<DT>(p.G, g + b);
      const double pmu = block_sum_f64(a, red) / n;
      double spq = 0, spp = 0;
      for (int64_t b = threadIdx.x; b < p.nbins; b += blockDim.x) {
        const double x = load1<DT>(p.Q, q * p.ldq + b) - qmu, y = load1<DT>(p.G, g + b) - pmu;
        spq = fma(x, y, spq);
        spp = fma(y, y, spp);
      }
      const double pq = block_sum_f64(spq, red), pp = block_sum_f64(spp, red);
      val = 1.0 - pq / (sqrt(pp) * sqrt(qq));   // 0 / 0 = NaN for a constant row, as numpy
    }
    if (threadIdx.x == 0) exact[c] = val;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const double dk = sort_and_write_wave<KC>(lists, exact, p.k, p.index_base, p.out_d + q * p.k, p.out_i + q * p.k);
    if (p.cert && threadIdx.x == 0) {
      // every row outside the KC candidates has a key >= tau, the KC-th candidate's, so its exact distance is
      // >= tau - bound (or NaN: key +inf); fewer than KC candidates means every row was re-ranked.  A constant
      // query (all NaN) and a tile voided by a wide uint32 count (tau = -inf) certify nothing.  The wave sort
      // ranks a NaN candidate behind the empty slots, so a k-th distance of +inf means a NaN (or k > N) within
      // the first k: left to the exact pass, which orders NaN rows as argsort does.
      const Cand last = lists[KC - 1];
      int ok = dk < __builtin_inf() && qq > 0.0;
      if (ok && last.i != CAND_EMPTY) ok = dk < (double)last.d - p.bound;
      p.cert[q] = ok;
    }
  }
}

template <int DT>
static int launch_general(hipStream_t st, const Args& a, const RerankArgs& m) {
  if (a.N > 0) {
    hipLaunchKernelGGL((ncc_tile_kernel<DT>), dim3((unsigned)(a.ntq * a.ntg)), dim3(256), 0, st, a);
    OFR_LAUNCH_CHECK("ncc_tile_kernel");
  }
  hipLaunchKernelGGL((ncc_rerank_kernel<DT>), dim3((unsigned)m.B), dim3(256), 0, st, m);
  OFR_LAUNCH_CHECK("ncc_rerank_kernel");
  return OFR_OK;
}

template <int DT, bool INTEGER>
static int launch_stats(hipStream_t st, const void* X, int64_t rows, int64_t ld, int64_t nbins, RowStat* out) {
  if (rows == 0) return OFR_OK;
  hipLaunchKernelGGL((ncc_stats_kernel<DT, INTEGER>), dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, st, X, rows, ld,
                     nbins, out);
  OFR_LAUNCH_CHECK("ncc_stats_kernel");
  return OFR_OK;
}

static int stats(hipStream_t st, int dtype, bool integer, const void* X, int64_t rows, int64_t ld, int64_t nbins,
                 RowStat* out) {
  switch (dtype) {
    case DT_U8: return integer ? launch_stats<DT_U8, true>(st, X, rows, ld, nbins, out)
                               : launch_stats<DT_U8, false>(st, X, rows, ld, nbins, out);
    case DT_U16: return integer ? launch_stats<DT_U16, true>(st, X, rows, ld, nbins, out)
                                : launch_stats<DT_U16, false>(st, X, rows, ld, nbins, out);
    case DT_U32: return launch_stats<DT_U32, false>(st, X, rows, ld, nbins, out);
    default: return launch_stats<DT_F32, false>(st, X, rows, ld, nbins, out);
  }
}

// workspace: tile lists [ceil(N / 64)][B][16] (the 64-row tiles; the MFMA pass has half as many), then the
// query and gallery row statistics
struct Ws {
  size_t sq, sg, bytes;
};
static Ws ws_layout(int64_t B, int64_t N) {
  Ws w;
  const int64_t T = cdiv(N > 0 ? N : 1, TT);
  w.sq = (size_t)round_up((int64_t)((size_t)T * (size_t)B * KC * sizeof(Cand)), 256);
  w.sg = w.sq + (size_t)round_up(B * (int64_t)sizeof(RowStat), 256);
  w.bytes = w.sg + (size_t)round_up((N > 0 ? N : 1) * (int64_t)sizeof(RowStat), 256) + 256;
  return w;
}

}  // namespace ncc
}  // namespace ofr

using namespace ofr;

extern "C" size_t ofr_ncorr_workspace_bytes(int64_t B, int64_t N, int k) {
  (void)k;   // the lists always hold 16 candidates
  return ncc::ws_layout(B > 0 ? B : 0, N).bytes;
}

extern "C" int ofr_ncorr_knn(void* stream, int dtype, const void* Q, int64_t B, int64_t ldq, const void* G, int64_t N,
                             int64_t ldg, int64_t nbins, int k, int64_t index_base, double* out_d, int64_t* out_i,
                             void* workspace, size_t workspace_bytes, int* cert) {
  using namespace ncc;
  OFR_CHECK_ARG(dtype >= DT_U8 && dtype <= DT_F32, "ofr_ncorr_knn: dtype must be 0 (u8), 1 (u16), 2 (u32) or 3 (f32)");
  OFR_CHECK_ARG(B >= 0 && N >= 0 && nbins >= 1, "ofr_ncorr_knn: bad sizes");
  if (k < 1 || k > OFR_MAX_K) return fail(OFR_E_UNSUPPORTED, "ofr_ncorr_knn: k must be in [1, 16]");
  if (B == 0) return OFR_OK;
  const int esz = dtype == DT_U8 ? 1 : dtype == DT_U16 ? 2 : 4;
  OFR_CHECK_ARG(Q && out_d && out_i && workspace, "ofr_ncorr_knn: null pointer");
  OFR_CHECK_ARG(ldq >= nbins && (ldq * esz) % 16 == 0 && ((uintptr_t)Q % 16) == 0,
                "ofr_ncorr_knn: query rows must be 16-byte aligned (ldq*elem % 16 == 0)");
  if (N > 0) {
    OFR_CHECK_ARG(G, "ofr_ncorr_knn: null gallery");
    OFR_CHECK_ARG(ldg >= nbins && (ldg * esz) % 16 == 0 && ((uintptr_t)G % 16) == 0,
                  "ofr_ncorr_knn: gallery rows must be 16-byte aligned (ldg*elem % 16 == 0)");
    OFR_CHECK_ARG(N < 0x7fffffffLL - MT, "ofr_ncorr_knn: N too large for one shard");
  }
  OFR_CHECK_ARG(((uintptr_t)workspace % 16) == 0, "ofr_ncorr_knn: workspace must be 16-byte aligned");
  OFR_CHECK_ARG(workspace_bytes >= ofr_ncorr_workspace_bytes(B, N, k), "ofr_ncorr_knn: workspace too small");
  // the MFMA pass while one int32 chain holds the row: 128 ceil(nbins / 128) 2^14 < 2^31
  const bool mfma = dtype == DT_U8 && round_up(nbins, BK) < (1LL << 17);
  // exact 64-bit statistics while nbins^2 max^2 < 2^63
  const bool integer = (dtype == DT_U8 && nbins < (1LL << 23)) || (dtype == DT_U16 && nbins < 46340);
  const int tile = mfma ? MT : TT;
  const Ws w = ws_layout(B, N);
  char* wsb = reinterpret_cast<char*>(workspace);
  Args a;
  a.Q = Q; a.B = B; a.ldq = ldq; a.G = G; a.N = N; a.ldg = ldg; a.nbins = nbins;
  a.sq = reinterpret_cast<RowStat*>(wsb + w.sq);
  a.sg = reinterpret_cast<RowStat*>(wsb + w.sg);
  a.cand = reinterpret_cast<Cand*>(wsb);
  a.ntq = cdiv(B, tile);
  a.ntg = N > 0 ? cdiv(N, tile) : 0;
  OFR_CHECK_ARG(a.ntq * a.ntg < 0x7fffffffLL, "ofr_ncorr_knn: grid too large");
  hipStream_t st = (hipStream_t)stream;
  int rc = stats(st, dtype, integer, Q, B, ldq, nbins, const_cast<RowStat*>(a.sq));
  if (rc != OFR_OK) return rc;
  rc = stats(st, dtype, integer, G, N, ldg, nbins, const_cast<RowStat*>(a.sg));
  if (rc != OFR_OK) return rc;
  // the absolute bound of the file header
  double bound = 2.0 * 0x1p-24 + 0x1p-40 + ((double)nbins + 16.0) * 0x1p-50;
  if (!mfma) bound += (double)nbins * 0x1p-24 < 0.0625 ? 1.0625 * ((double)nbins + 2.0) * 0x1p-24 : 4.0;
  RerankArgs m{a.cand, a.ntg, B, Q, ldq, G, ldg, nbins, k, index_base, out_d, out_i, cert, bound};
  if (mfma) {
    if (N > 0) {
      hipLaunchKernelGGL(ncc_mfma_kernel, dim3((unsigned)(a.ntq * a.ntg)), dim3(256), 0, st, a);
      OFR_LAUNCH_CHECK("ncc_mfma_kernel");
    }
    hipLaunchKernelGGL((ncc_rerank_kernel<DT_U8>), dim3((unsigned)B), dim3(256), 0, st, m);
    OFR_LAUNCH_CHECK("ncc_rerank_kernel");
    return OFR_OK;
  }
  switch (dtype) {
    case DT_U8: return launch_general<DT_U8>(st, a, m);
    case DT_U16: return launch_general<DT_U16>(st, a, m);
    case DT_U32: return launch_general<DT_U32>(st, a, m);
    default: return launch_general<DT_F32>(st, a, m);
  }
}
