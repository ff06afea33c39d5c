// results2json on the device (kgdet_amd/evaluation_device.py: write_device_results_json) for gfx950: the text of
// P.bbox.json / P.keypoints.json, byte for byte what json.dump writes for kpt2json's lists, from the [N, M, 7 + 3K] float32
// tensor the detections lie in (runner.DeviceResults.rows) and what kgdet_coco_order_dets left of them (vals: xywh and the
// score rounded like Python's round; info: a row's index k in the host enumeration).  Record r = img_base[image] + k.
//
// A value is an integer q = |value| * 10^d < 2^40 + 1 and a sign: q = rint(|v| * 10^d) for a landmark value (the float32 x
// 10^d product is exact in float64, so this IS np.round's rint) and for a rounded xywh / score double (n / 10^d * 10^d is
// within 2^-12 of n).  Its text is repr of that double: [-] integer digits . fractional digits without trailing zeros, at
// least one; at most 15 bytes.  A value outside the domain (not finite, |v| * 10^d >= 2^40) is counted by the measure kernel
// and stands as 0.0 in both kernels, so lengths and text always agree; the caller refuses such a set.
//
// kgdet_coco_json_measure: one workgroup per image, one wave per row: the lanes stride over the 3K landmark values and the
// value lengths are summed over the wave by shuffles; lane 0 writes both record lengths and the record's source row.
// kgdet_coco_json_write: one workgroup per record (256 threads for a keypoints record, one wave for a bbox record).  The
// record, with the ", " that separates it from its predecessor, is assembled in LDS: a thread owns a run of consecutive
// values, the runs' byte lengths are scanned over the workgroup (wave shuffles + one pass over the wave totals), every thread
// then writes its digits at its place.  The LDS image starts (destination address mod 16) bytes into the buffer, so its
// 16-byte chunks are the destination's aligned chunks: whole chunks leave as one ds_read_b128 + one 16-byte global store per
// lane (consecutive lanes, consecutive chunks: conflict-free reads, coalesced stores), the unaligned head and tail chunk as
// byte stores.  A record whose assembled length differs from offset[r + 1] - offset[r], or whose place lies outside the
// range's bytes, is not written and counted in flags[1].
// LDS per workgroup: 16 (alignment shift) + 128 (frame: literals, two ", ", ids of up to 20 digits) + 3K * 17 (15 bytes per
// value and its ", "), rounded up to 16, as dynamic LDS, plus 32 bytes of wave totals.  K = 294: 15 152 bytes, ten workgroups
// fit a CU's 160 KiB (the 256-thread occupancy limit is eight).  K <= KGDET_COCO_JSON_MAX_K = 1024 (52 384 bytes) keeps it
// below the 64 KiB a workgroup gets without asking.
// Integer arithmetic and single float64 operations; no float atomics; plain C++ and vector stores only.
#include "common.h"

#pragma clang fp contract(off)

namespace kgdet {

namespace {

constexpr int kWave = 64;
constexpr int kThreadsImg = 256;       // measure: four rows of an image at a time
constexpr int kVals = 6, kInfo = 3;    // (coco_pack_dets.hip's vals / info rows)
constexpr int kFrame = 128;            // bytes a record holds beside its values and their separators
constexpr double kLimit = 1099511627776.0;       // 2^40

typedef unsigned long long u64;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct Value {
  u64 q;
  bool neg;
};

// a landmark value: widened, q = rint(|v| * S); *bad is raised outside the domain
__device__ __forceinline__ Value value_of_float(float v, double S, int *bad) {
  const double p = fabs((double)v) * S;
  if (!(p < kLimit)) {
    *bad += 1;
    return Value{0, false};
  }
  return Value{(u64)rint(p), (__float_as_uint(v) >> 31) != 0};
}

// a double kgdet_coco_order_dets rounded: n / S with n <= 2^40
__device__ __forceinline__ Value value_of_rounded(double x, double S) {
  const double p = fabs(x) * S;
  if (!(p < kLimit + 1.0)) return Value{0, false};
  return Value{(u64)rint(p), (__double_as_longlong(x) >> 63) != 0};
}

__device__ __forceinline__ int digits_u32(unsigned v) {
  int n = 1;
  if (v >= 10u) n = 2;
  if (v >= 100u) n = 3;
  if (v >= 1000u) n = 4;
  if (v >= 10000u) n = 5;
  if (v >= 100000u) n = 6;
  if (v >= 1000000u) n = 7;
  if (v >= 10000000u) n = 8;
  if (v >= 100000000u) n = 9;
  if (v >= 1000000000u) n = 10;
  return n;
}

__device__ __forceinline__ int digits_u64(u64 v) {
  if (v < 1000000000ull) return digits_u32((unsigned)v);
  if (v < 1000000000000000000ull) return 9 + digits_u32((unsigned)(v / 1000000000ull));
  return v < 10000000000000000000ull ? 19 : 20;
}

// q = ip * 10^d + fr
__device__ __forceinline__ void split_decimal(u64 q, int d, u64 *ip, unsigned *fr) {
  switch (d) {
    case 1: *ip = q / 10ull; *fr = (unsigned)(q % 10ull); break;
    case 2: *ip = q / 100ull; *fr = (unsigned)(q % 100ull); break;
    case 3: *ip = q / 1000ull; *fr = (unsigned)(q % 1000ull); break;
    default: *ip = q / 10000ull; *fr = (unsigned)(q % 10000ull); break;
  }
}

// fractional digits kept (>= 1) and the fraction without its trailing zeros
__device__ __forceinline__ int strip_fraction(unsigned *fr, int d) {
  int nf = d;
  while (nf > 1 && *fr % 10u == 0u) {
    *fr /= 10u;
    nf -= 1;
  }
  return nf;
}

__device__ __forceinline__ int value_length(Value v, int d) {
  u64 ip;
  unsigned fr;
  split_decimal(v.q, d, &ip, &fr);
  return (v.neg ? 1 : 0) + digits_u64(ip) + 1 + strip_fraction(&fr, d);
}

// the decimal digits of v, n of them, ending before s[end]
__device__ __forceinline__ void put_digits(unsigned char *s, int end, u64 v, int n) {
  for (int i = 0; i < n; ++i) {
    s[end - 1 - i] = (unsigned char)('0' + (unsigned)(v % 10ull));
    v /= 10ull;
  }
}

// -> the position behind the value's text
__device__ __forceinline__ int put_value(unsigned char *s, int pos, Value v, int d) {
  u64 ip;
  unsigned fr;
  split_decimal(v.q, d, &ip, &fr);
  const int nf = strip_fraction(&fr, d), ni = digits_u64(ip);
  if (v.neg) s[pos++] = '-';
  put_digits(s, pos + ni, ip, ni);
  pos += ni;
  s[pos++] = '.';
  put_digits(s, pos + nf, fr, nf);
  return pos + nf;
}

template <int N>
__device__ __forceinline__ int put_text(unsigned char *s, int pos, const char (&text)[N]) {
  for (int i = 0; i < N - 1; ++i) s[pos + i] = (unsigned char)text[i];
  return pos + N - 1;
}

__device__ __forceinline__ int put_id(unsigned char *s, int pos, u64 v) {
  const int n = digits_u64(v);
  put_digits(s, pos + n, v, n);
  return pos + n;
}

#define KGDET_JSON_HEAD "{\"image_id\": "
#define KGDET_JSON_BBOX ", \"bbox\": ["
#define KGDET_JSON_KPTS ", \"keypoints\": ["
#define KGDET_JSON_SCORE "], \"score\": "
#define KGDET_JSON_CAT ", \"category_id\": "
constexpr int kHeadLen = sizeof(KGDET_JSON_HEAD) - 1, kBboxLen = sizeof(KGDET_JSON_BBOX) - 1, kKptsLen = sizeof(KGDET_JSON_KPTS) - 1;
constexpr int kScoreLen = sizeof(KGDET_JSON_SCORE) - 1, kCatLen = sizeof(KGDET_JSON_CAT) - 1;
static_assert(2 + kHeadLen + 20 + kKptsLen + kScoreLen + 15 + kCatLen + 20 + 1 <= kFrame, "the frame budget of a keypoints record");
constexpr int kBboxSlots = 16;         // a bbox record's buffer is that of a record of 16 values
static_assert(2 + kHeadLen + 20 + kBboxLen + 4 * 17 + kScoreLen + 15 + kCatLen + 20 + 1 <= kFrame + kBboxSlots * 17,
              "a bbox record fits its buffer");

__device__ __forceinline__ int wave_sum(int v) {
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

__global__ __launch_bounds__(kThreadsImg) void coco_json_measure_kernel(
    const float *__restrict__ rows, int M, int W, const double *__restrict__ vals, const int *__restrict__ info,
    const long long *__restrict__ img_base, const long long *__restrict__ img_ids, const long long *__restrict__ cat_ids, int L,
    int d, double S, int *__restrict__ len_bbox, int *__restrict__ len_kp, long long *__restrict__ rec_src, long long n_records,
    int *__restrict__ flags) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const long long img = blockIdx.x;
  const float *src = rows + img * (long long)M * W;
  const float cf = src[6];
  if (!(cf >= 0.0f && cf < (float)(M + 1))) return;      // (counted by the order kernel)
  const int count = (int)cf;
  const double *v_in = vals + img * (long long)M * kVals;
  const int *i_in = info + img * (long long)M * kInfo;
  const long long base = img_base[img];
  const int id_digits = digits_u64((u64)img_ids[img]);
  const int n_f = W - 7;
  int bad = 0, misplaced = 0;
  for (int i = wave; i < count; i += kThreadsImg / kWave) {
    const int k = i_in[i * kInfo + 1];
    if (k < 0) continue;                                   // (wave-uniform: a row bbox2result_kp drops)
    const float *r = src + (long long)i * W;
    const int label = (int)r[5];
    const long long rec = base + k;
    if (label < 0 || label >= L || rec < 0 || rec >= n_records) {
      misplaced += lane == 0 ? 1 : 0;
      continue;
    }
    int sum = 0;
    for (int j = lane; j < n_f; j += kWave) sum += value_length(value_of_float(r[7 + j], S, &bad), d);
    sum = wave_sum(sum);
    if (lane == 0) {
      const double *v = v_in + (long long)i * kVals;
      const int tail = kScoreLen + value_length(value_of_rounded(v[4], S), d) + kCatLen + digits_u64((u64)cat_ids[label]) + 1;
      int box = 0;
      for (int c = 0; c < 4; ++c) box += value_length(value_of_rounded(v[c], S), d);
      len_bbox[rec] = kHeadLen + id_digits + kBboxLen + box + 2 * 3 + tail;
      len_kp[rec] = kHeadLen + id_digits + kKptsLen + sum + 2 * (n_f - 1) + tail;
      rec_src[rec] = img * M + i;
    }
  }
  if (bad) atomicAdd(&flags[0], bad);
  if (misplaced) atomicAdd(&flags[1], misplaced);
}

// kKind 0: bbox records (four values from vals), 1: keypoints records (3K values from the row)
template <int kKind, int kThreads>
__global__ __launch_bounds__(kThreads) void coco_json_write_kernel(
    const float *__restrict__ rows, long long n_rows, int W, const double *__restrict__ vals, const long long *__restrict__ rec_src,
    const long long *__restrict__ offset, const long long *__restrict__ img_ids, const long long *__restrict__ cat_ids, int M, int L,
    int d, double S, long long r0, long long range_bytes, unsigned char *__restrict__ out, int lds_bytes, int *__restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_rec[];
  __shared__ int s_wave[kThreads / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const long long rec = r0 + blockIdx.x;
  const long long at = offset[rec] - offset[r0], want = offset[rec + 1] - offset[rec];
  const long long row = rec_src[rec];
  bool ok = row >= 0 && row < n_rows && at >= 0 && want > 0 && want <= range_bytes - at;
  int label = -1;
  if (ok) {
    label = (int)rows[row * W + 5];
    ok = label >= 0 && label < L;
  }
  if (!ok) {                                               // (uniform over the workgroup)
    if (tid == 0) atomicAdd(&flags[1], 1);
    return;
  }
  const float *r = rows + row * W;
  const double *v = vals + row * kVals;
  const u64 img_id = (u64)img_ids[row / M], cat_id = (u64)cat_ids[label];
  unsigned char *dst = out + at;
  const int shift = (int)((uintptr_t)dst & 15u);
  const int n_v = kKind ? W - 7 : 4;
  const int per = (n_v + kThreads - 1) / kThreads;         // values of a thread: [j0, j1), consecutive
  const int j0 = min(tid * per, n_v), j1 = min(j0 + per, n_v);
  int bad = 0;                                             // (the measure kernel's to count)
  int mine = 0;
  for (int j = j0; j < j1; ++j)
    mine += value_length(kKind ? value_of_float(r[7 + j], S, &bad) : value_of_rounded(v[j], S), d) + (j + 1 < n_v ? 2 : 0);
  int scan = mine;                                         // inclusive over the wave, then the waves before it
  for (int off = 1; off < kWave; off <<= 1) {
    const int o = __shfl_up(scan, off, kWave);
    if (lane >= off) scan += o;
  }
  if (lane == kWave - 1) s_wave[wave] = scan;
  __syncthreads();
  int before = scan - mine, total = 0;
  for (int w = 0; w < kThreads / kWave; ++w) {
    if (w < wave) before += s_wave[w];
    total += s_wave[w];
  }
  const int sep = rec > 0 ? 2 : 0;
  const int head = sep + kHeadLen + digits_u64(img_id) + (kKind ? kKptsLen : kBboxLen);
  const Value score = value_of_rounded(v[4], S);
  const int length = head + total + kScoreLen + value_length(score, d) + kCatLen + digits_u64(cat_id) + 1;
  if (length != want || shift + length > lds_bytes) {
    if (tid == 0) atomicAdd(&flags[1], 1);
    return;
  }
  unsigned char *s = s_rec + shift;
  if (tid == 0) {
    int pos = 0;
    if (sep) pos = put_text(s, pos, ", ");
    pos = put_text(s, pos, KGDET_JSON_HEAD);
    pos = put_id(s, pos, img_id);
    if (kKind) put_text(s, pos, KGDET_JSON_KPTS); else put_text(s, pos, KGDET_JSON_BBOX);
  }
  if (tid == kThreads - 1) {
    int pos = head + total;
    pos = put_text(s, pos, KGDET_JSON_SCORE);
    pos = put_value(s, pos, score, d);
    pos = put_text(s, pos, KGDET_JSON_CAT);
    pos = put_id(s, pos, cat_id);
    s[pos] = '}';
  }
  int pos = head + before;
  for (int j = j0; j < j1; ++j) {
    pos = put_value(s, pos, kKind ? value_of_float(r[7 + j], S, &bad) : value_of_rounded(v[j], S), d);
    if (j + 1 < n_v) pos = put_text(s, pos, ", ");
  }
  __syncthreads();
  // copy-out: chunk c is s_rec[16c, 16c + 16) and the destination's aligned 16 bytes at dst - shift + 16c
  const int end = shift + length, n_chunks = (end + 15) / 16;
  unsigned char *gbase = dst - shift;
  for (int c = tid; c < n_chunks; c += kThreads) {
    const int lo = 16 * c;
    if (lo >= shift && lo + 16 <= end) {
      *reinterpret_cast<u32x4 *>(gbase + lo) = *reinterpret_cast<const u32x4 *>(s_rec + lo);
    } else {
      const int b0 = max(lo, shift), b1 = min(lo + 16, end);
      for (int b = b0; b < b1; ++b) gbase[b] = s_rec[b];
    }
  }
}

const double kPow10[5] = {1e0, 1e1, 1e2, 1e3, 1e4};

size_t record_lds_bytes(int n_values) { return align_up((size_t)16 + kFrame + (size_t)n_values * 17, 16); }

}  // namespace

}  // namespace kgdet

using namespace kgdet;

extern "C" {

int kgdet_coco_json_measure(const float *rows, int64_t N, int32_t M, int32_t W, const double *vals, const int32_t *info,
                            const int64_t *img_base, const int64_t *img_ids, const int64_t *cat_ids, int32_t L,
                            int32_t num_digits, int32_t *len_bbox, int32_t *len_kp, int64_t *rec_src, int64_t n_records,
                            int32_t *flags, void *stream) {
  KGDET_CHECK_SHAPE(num_digits >= 1 && num_digits <= 4, "coco_json_measure: num_digits %d (1 .. 4)", num_digits);
  KGDET_CHECK_SHAPE(M >= 1 && M <= KGDET_COCO_ORDER_MAX_ROWS, "coco_json_measure: %d rows per image (1 .. %d)", M,
                    KGDET_COCO_ORDER_MAX_ROWS);
  KGDET_CHECK_SHAPE(W >= 10 && (W - 7) % 3 == 0 && (W - 7) / 3 <= KGDET_COCO_JSON_MAX_K,
                    "coco_json_measure: rows of %d floats (7 + 3K, K = 1 .. %d)", W, KGDET_COCO_JSON_MAX_K);
  KGDET_CHECK_SHAPE(L >= 1 && L <= KGDET_COCO_ORDER_MAX_LABELS, "coco_json_measure: %d labels (1 .. %d)", L,
                    KGDET_COCO_ORDER_MAX_LABELS);
  KGDET_CHECK_SHAPE(N >= 0 && N < (1ll << 31) && n_records >= 0, "coco_json_measure: %lld images (0 .. 2^31 - 1), %lld records",
                    (long long)N, (long long)n_records);
  if (N == 0) return KGDET_OK;
  KGDET_CHECK_SHAPE(rows && vals && info && img_base && img_ids && cat_ids && flags && (n_records == 0 || (len_bbox && len_kp && rec_src)),
                    "coco_json_measure: null pointer");
  hipLaunchKernelGGL(coco_json_measure_kernel, dim3((unsigned)N), dim3(kThreadsImg), 0, (hipStream_t)stream, rows, (int)M, (int)W,
                     vals, (const int *)info, (const long long *)img_base, (const long long *)img_ids, (const long long *)cat_ids,
                     (int)L, (int)num_digits, kPow10[num_digits], (int *)len_bbox, (int *)len_kp, (long long *)rec_src,
                     (long long)n_records, (int *)flags);
  KGDET_CHECK_LAUNCH("coco_json_measure_kernel");
  return KGDET_OK;
}

int kgdet_coco_json_write(int32_t kind, const float *rows, int64_t N, int32_t M, int32_t W, const double *vals,
                          const int64_t *rec_src, const int64_t *offset, const int64_t *img_ids, const int64_t *cat_ids,
                          int32_t L, int32_t num_digits, int64_t r0, int64_t r1, int64_t range_bytes, uint8_t *out,
                          int64_t out_bytes, int32_t *flags, void *stream) {
  KGDET_CHECK_SHAPE(kind == 0 || kind == 1, "coco_json_write: kind %d (0 bbox, 1 keypoints)", kind);
  KGDET_CHECK_SHAPE(num_digits >= 1 && num_digits <= 4, "coco_json_write: num_digits %d (1 .. 4)", num_digits);
  KGDET_CHECK_SHAPE(M >= 1 && M <= KGDET_COCO_ORDER_MAX_ROWS, "coco_json_write: %d rows per image (1 .. %d)", M,
                    KGDET_COCO_ORDER_MAX_ROWS);
  KGDET_CHECK_SHAPE(W >= 10 && (W - 7) % 3 == 0 && (W - 7) / 3 <= KGDET_COCO_JSON_MAX_K,
                    "coco_json_write: rows of %d floats (7 + 3K, K = 1 .. %d: a record is assembled in LDS)", W,
                    KGDET_COCO_JSON_MAX_K);
  KGDET_CHECK_SHAPE(L >= 1 && L <= KGDET_COCO_ORDER_MAX_LABELS, "coco_json_write: %d labels (1 .. %d)", L, KGDET_COCO_ORDER_MAX_LABELS);
  KGDET_CHECK_SHAPE(N >= 0 && N < (1ll << 31), "coco_json_write: %lld images (0 .. 2^31 - 1)", (long long)N);
  KGDET_CHECK_SHAPE(r0 >= 0 && r1 >= r0, "coco_json_write: records [%lld, %lld)", (long long)r0, (long long)r1);
  KGDET_CHECK_SHAPE(range_bytes >= 0 && out_bytes >= range_bytes, "coco_json_write: %lld bytes of output for a range of %lld",
                    (long long)out_bytes, (long long)range_bytes);
  if (N == 0 || r1 == r0) return KGDET_OK;
  KGDET_CHECK_SHAPE(r1 <= N * (int64_t)M && r1 - r0 < (1ll << 31),
                    "coco_json_write: records [%lld, %lld) of at most %lld (and fewer than 2^31 in a call)", (long long)r0,
                    (long long)r1, (long long)(N * (int64_t)M));
  KGDET_CHECK_SHAPE(rows && vals && rec_src && offset && img_ids && cat_ids && out && flags, "coco_json_write: null pointer");
  const long long n_rows = (long long)N * M;
  const unsigned grid = (unsigned)(r1 - r0);
  if (kind == 1) {
    const size_t lds = record_lds_bytes(W - 7);
    hipLaunchKernelGGL((coco_json_write_kernel<1, 256>), dim3(grid), dim3(256), lds, (hipStream_t)stream, rows, n_rows, (int)W, vals,
                       (const long long *)rec_src, (const long long *)offset, (const long long *)img_ids,
                       (const long long *)cat_ids, (int)M, (int)L, (int)num_digits, kPow10[num_digits], (long long)r0,
                       (long long)range_bytes, (unsigned char *)out, (int)lds, (int *)flags);
  } else {
    const size_t lds = record_lds_bytes(kBboxSlots);
    hipLaunchKernelGGL((coco_json_write_kernel<0, 64>), dim3(grid), dim3(64), lds, (hipStream_t)stream, rows, n_rows, (int)W, vals,
                       (const long long *)rec_src, (const long long *)offset, (const long long *)img_ids,
                       (const long long *)cat_ids, (int)M, (int)L, (int)num_digits, kPow10[num_digits], (long long)r0,
                       (long long)range_bytes, (unsigned char *)out, (int)lds, (int *)flags);
  }
  KGDET_CHECK_LAUNCH("coco_json_write_kernel");
  return KGDET_OK;
}

}  // extern "C"
