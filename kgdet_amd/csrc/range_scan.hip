// Range scan of a whole model's worth of fp32 tensors in one kernel launch (gfx950): per tensor the largest finite |v * s|, the
// number of non-finite products and the numbers of products beyond two limits -- what kgdet_amd/numerics.py needs to tell
// whether the operands of the fp16-part dense convolutions (dense_common.h, "FORWARD operands") sit inside their envelope:
// |w * s| * 2^8 <= 65504 for a (folded) weight, |x| <= 65504 (fp32-class) / 131008 (11 bits) for an activation.
//
// No reference counterpart (the reference computes its convolutions in fp32 and has no envelope to leave).
//
// Table row per tensor, 8 x int64 (include/kgdet_hip.h kgdet_range_scan_multi):
//   {tensor, count, inner, gamma or 0, var or 0, bits of eps, bits of hi1 | bits of hi2 << 32, first block}
// inner > 0: element i belongs to scale row i / inner and s = gamma[row] / sqrtf(var[row] + eps) (gamma 0: 1 / sqrtf(...)) is
// formed HERE, from the BatchNorm's own tensors: the scan needs no torch ops and no folded copy of the weight.  inner == 0: s = 1
// and the product is the value itself (no multiplication: the maximum is the bit pattern of an element).
// Record per row, 4 x uint32, zeroed by the call and then only raised / counted up with INTEGER atomics (the bit pattern of a
// non-negative finite float orders like the float): maxima and integer counts do not depend on the order of arrival, so the
// record is the same for every schedule.  No float atomics.
//
// Memory-bound, one pass: 16-byte loads from the first 16-byte boundary of the tensor on (tensors are only 4-byte aligned:
// slices of flat buffers, odd-sized parameters behind one another), the up-to-three elements in front of it and behind the last
// whole quad as scalars; a block takes chunks of kScanChunk elements (256 threads x 4 x float4, all four loads issued before the
// first use) and a row gets at most kScanRowBlocks blocks, which stride over its chunks -- 44 VGPRs, no scratch, 8 waves per SIMD.
#include <float.h>

#include "common.h"

namespace kgdet {

namespace {
constexpr int kScanChunk = 4096;      // elements per block and trip (256 threads x 4 x float4)
constexpr int kScanRowBlocks = 256;   // blocks per row at most: one per CU; longer rows stride
constexpr int kScanRowWords = 8;

__host__ __device__ inline long long scan_blocks(long long count) {
  const long long b = (count + kScanChunk - 1) / kScanChunk;
  return b < 1 ? 1 : (b > kScanRowBlocks ? kScanRowBlocks : b);
}

__device__ __forceinline__ const long long *scan_row(const long long *__restrict__ table, int n, int block) {
  int lo = 0, hi = n - 1;   // uniform binary search on the first-block column
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int)table[mid * kScanRowWords + 7] <= block) lo = mid; else hi = mid - 1;
  }
  return table + lo * kScanRowWords;
}

struct ScanAcc {
  float mx;
  unsigned bad, over1, over2;
};

struct ScanRow {
  const float *gamma, *var;
  float eps, hi1, hi2;
  long long inner;
  bool narrow;   // every index of the row fits 32 bits: the row-of-element division is a 32-bit one

  __device__ __forceinline__ float scale(long long r) const {
    const float g = gamma ? gamma[r] : 1.0f;
    return g / sqrtf(var[r] + eps);     // (correctly rounded, both: hipcc's default for fp32 sqrt and division)
  }
  __device__ __forceinline__ long long row_of(long long i) const {
    return narrow ? (long long)((unsigned)i / (unsigned)inner) : i / inner;
  }
};

__device__ __forceinline__ void scan_take(ScanAcc &a, float p, const ScanRow &r) {
  const float m = fabsf(p);
  if (m <= FLT_MAX) a.mx = fmaxf(a.mx, m); else ++a.bad;     // (NaN and inf fail the comparison)
  a.over1 += m > r.hi1 ? 1u : 0u;                             // (inf counts, NaN does not)
  a.over2 += m > r.hi2 ? 1u : 0u;
}

// `k` consecutive elements from index i on (k <= 4), each with the scale of its own row
template <bool SCALED>
__device__ __forceinline__ void scan_run(ScanAcc &a, const float *v, int k, long long i, const ScanRow &r) {
  if constexpr (!SCALED) {
    for (int e = 0; e < k; ++e) scan_take(a, v[e], r);
  } else {
    long long row = r.row_of(i), rem = i - row * r.inner;
    float s = r.scale(row);
    for (int e = 0; e < k; ++e) {
      while (rem >= r.inner) {     // (inner < 4: a quad may span several rows)
        rem -= r.inner;
        s = r.scale(++row);
      }
      scan_take(a, v[e] * s, r);
      ++rem;
    }
  }
}

template <bool SCALED>
__device__ __forceinline__ void scan_tensor(ScanAcc &a, const float *__restrict__ p, long long count, int local, int blocks,
                                            const ScanRow &r) {
  long long head = (long long)((16 - (reinterpret_cast<size_t>(p) & 15)) & 15) >> 2;   // elements in front of the 16-byte boundary
  if (head > count) head = count;
  const long long quads = (count - head) >> 2, tail = count - head - 4 * quads;
  const float *body = p + head;
  for (long long c = local; c * (kScanChunk / 4) < quads; c += blocks) {
    float4 v[4];
    long long q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      q[k] = c * (kScanChunk / 4) + k * 256 + threadIdx.x;
      if (q[k] < quads) v[k] = *reinterpret_cast<const float4 *>(body + 4 * q[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (q[k] < quads) {
        const float e[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
        scan_run<SCALED>(a, e, 4, head + 4 * q[k], r);
      }
    }
  }
  if (local == 0) {      // the scalar head (lanes of wave 0) and tail (lanes of wave 1) of the row
    if ((long long)threadIdx.x < head) scan_run<SCALED>(a, p + threadIdx.x, 1, threadIdx.x, r);
    const long long t = (long long)threadIdx.x - 64;
    if (t >= 0 && t < tail) scan_run<SCALED>(a, body + 4 * quads + t, 1, head + 4 * quads + t, r);
  }
}
}  // namespace

__global__ __launch_bounds__(256) void range_scan_multi(const long long *__restrict__ table, int n, unsigned *__restrict__ records) {
  __shared__ unsigned red[4][4];
  const long long *row = scan_row(table, n, blockIdx.x);
  const float *p = reinterpret_cast<const float *>(row[0]);
  const long long count = row[1];
  ScanRow r;
  r.inner = row[2];
  r.gamma = reinterpret_cast<const float *>(row[3]);
  r.var = reinterpret_cast<const float *>(row[4]);
  r.eps = __uint_as_float((unsigned)row[5]);
  r.hi1 = __uint_as_float((unsigned)row[6]);
  r.hi2 = __uint_as_float((unsigned)((unsigned long long)row[6] >> 32));
  r.narrow = count <= 0xffffffffLL;
  const int local = (int)blockIdx.x - (int)row[7], blocks = (int)scan_blocks(count);
  ScanAcc a = {0.f, 0u, 0u, 0u};
  if (local < blocks && count > 0) {
    if (r.inner > 0 && r.var != nullptr) scan_tensor<true>(a, p, count, local, blocks, r);
    else scan_tensor<false>(a, p, count, local, blocks, r);
  }
  unsigned w[4] = {__float_as_uint(a.mx), a.bad, a.over1, a.over2};
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)w[0], d);
    w[0] = o > w[0] ? o : w[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) w[j] += (unsigned)__shfl_xor((int)w[j], d);
  }
  if ((threadIdx.x & 63) == 0)
    for (int j = 0; j < 4; ++j) red[threadIdx.x >> 6][j] = w[j];
  __syncthreads();
  if (threadIdx.x < 4) {
    const int j = threadIdx.x;
    unsigned *out = records + (size_t)((row - table) / kScanRowWords) * 4;
    if (j == 0) {
      unsigned m = red[0][0];
      for (int k = 1; k < 4; ++k) m = red[k][0] > m ? red[k][0] : m;
      if (m) atomicMax(out, m);
    } else {
      const unsigned s = red[0][j] + red[1][j] + red[2][j] + red[3][j];
      if (s) atomicAdd(out + j, s);
    }
  }
}

}  // namespace kgdet

using namespace kgdet;

extern "C" int32_t kgdet_range_scan_chunk(void) { return kScanChunk; }

extern "C" int64_t kgdet_range_scan_blocks(int64_t count) { return scan_blocks(count); }

extern "C" int kgdet_range_scan_multi(const int64_t *table_dev, int32_t n_rows, int64_t total_blocks, uint32_t *records,
                                      void *stream) {
  KGDET_CHECK_SHAPE(table_dev && records && n_rows > 0 && total_blocks > 0 && total_blocks < (1LL << 31), "bad arguments");
  KGDET_CHECK_SHAPE(total_blocks <= (int64_t)n_rows * kScanRowBlocks, "more blocks than the rows can have");
  KGDET_HIP_TRY(hipMemsetAsync(records, 0, (size_t)n_rows * 4 * sizeof(uint32_t), (hipStream_t)stream));
  hipLaunchKernelGGL(range_scan_multi, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                     (const long long *)table_dev, n_rows, records);
  KGDET_CHECK_LAUNCH("range_scan_multi");
  return KGDET_OK;
}
