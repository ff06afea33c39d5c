// C-ABI launchers for deformable convolution (see include/kgdet_hip.h for the contract and the
// reference entry points each one replaces).
//
// Layout of this file: shape derivation, eligibility and table sizes (pure arithmetic, shared by the size queries and the
// launchers), then the group / sub-problem builders, then the entry points: packers, forward, grad_input / grad_offset,
// grad_weight and the two dispatchers.
//
// Environment switches (A/B measurement and test hooks, none is part of the API).  "cached": read once per process.
//   KGDET_DCN_ROUNDS=n        cached    plan_static_ranges: rounds of the multi-round static schedule (0 = its own rule)
//   KGDET_DCN_STREAMK         cached    set (any value): no static schedule, stream-K everywhere it is optional
//   KGDET_DCN_FULL_GRID       cached    set (any value): small groups run on the full grid (small_launch_grid)
//   KGDET_DCN_CHAIN_DMA=0     cached    forward: no blocked input copy (plane hand-over through registers)
//   KGDET_DCN_OFFSET_PAIR=0   cached    grad_offset: dcn_bwd_offset_plane<2> instead of the tap-pair kernel
//   KGDET_DCN_OFFSET_XBLK=0   cached    grad_offset tap-pair kernel: no blocked input copy
//   KGDET_DCN_SUMS_XCD=0      cached    grouped backward: sums kernels dealt in launch order, not per XCD (also: no hot GEMM)
//   KGDET_DCN_SUMS_HALVES=1   cached    grouped backward: (experiment, off) every (problem, image) as two XCD segments
//   KGDET_DCN_HOT_GEMM=0      cached    grouped backward: hot cells through the cluster kernel instead of dcn_hot_gemm
//   KGDET_DCN_BWD_PREPARE=0   cached    grouped backward: record builder and pixel-major copy as two launches
//   KGDET_DCN_WGRAD_OS=0      cached    grad_weight: stream-K kernel + fix-up instead of the output-stationary kernel
//   KGDET_DCN_HOT_MAX_COLS=n  per call  (test) a shorter hot-column list, to reach the overflow rule with small kernels
//   KGDET_DCN_HOT_DEBUG=1     per call  (test) record the hot-column counts for kgdet_debug_dcn_hot_columns
#include "common.h"
#include <algorithm>
#include <vector>

#include "dcn_kernels.h"

namespace kgdet {

namespace {

constexpr size_t kMaxLds = 160 * 1024;

// ---------------------------------------------------------------------------------------------------------------------
// Shapes, eligibility, table sizes
// ---------------------------------------------------------------------------------------------------------------------
struct Derived {
  int Ho, Wo, K, Cg, Og, Cg_pad, Og_pad;
  int Og_pad16, Cg_pad256;  // transposed image for backward-input
  size_t fwd_image_floats() const { return (size_t)K * Cg_pad * Og_pad; }
  size_t bwd_image_floats() const { return (size_t)K * Og_pad16 * Cg_pad256; }
  // bf16 hi/lo image of the plane forward kernel: same element count, 2 x 2 bytes each
  size_t plane_image_floats() const { return (size_t)K * Cg_pad * Og_pad; }
  // its transpose (rows = input channels) for the plane grad_input kernel
  size_t plane_t_image_floats() const { return (size_t)K * Og_pad16 * Cg_pad256; }
};

// channels of the output buffer the convolution writes its window of
int o_total(const kgdet_dcn_shape *s) { return s->out_channels_total > 0 ? s->out_channels_total : s->O; }

int derive(const kgdet_dcn_shape *s, Derived &d) {
  // the reference's shape_check (mmdet/ops/dcn/src/deform_conv_cuda.cpp:61-149)
  KGDET_CHECK_SHAPE(s != nullptr, "null shape");
  KGDET_CHECK_SHAPE(s->kh > 0 && s->kw > 0, "kernel size should be greater than zero, but got kH: %d kW: %d",
                    s->kh, s->kw);
  KGDET_CHECK_SHAPE(s->stride_h > 0 && s->stride_w > 0, "stride should be greater than zero, but got dH: %d dW: %d",
                    s->stride_h, s->stride_w);
  KGDET_CHECK_SHAPE(s->dil_h > 0 && s->dil_w > 0,
                    "dilation should be greater than 0, but got dilationH: %d dilationW: %d", s->dil_h, s->dil_w);
  KGDET_CHECK_SHAPE(s->N > 0 && s->C > 0 && s->O > 0 && s->H > 0 && s->W > 0, "empty tensor dimension");
  KGDET_CHECK_SHAPE(s->groups > 0 && s->C % s->groups == 0 && s->O % s->groups == 0,
                    "channels must divide groups (C=%d O=%d groups=%d)", s->C, s->O, s->groups);
  KGDET_CHECK_SHAPE(s->deformable_groups > 0 && s->C % s->deformable_groups == 0,
                    "input channels must divide deformable group size");
  KGDET_CHECK_SHAPE(s->out_channel_offset >= 0 &&
                        (s->out_channels_total == 0 ? s->out_channel_offset == 0
                                                    : s->out_channel_offset + s->O <= s->out_channels_total),
                    "output channel window [%d, %d) does not fit %d channels", s->out_channel_offset,
                    s->out_channel_offset + s->O, s->out_channels_total);
  d.Ho = (s->H + 2 * s->pad_h - (s->dil_h * (s->kh - 1) + 1)) / s->stride_h + 1;
  d.Wo = (s->W + 2 * s->pad_w - (s->dil_w * (s->kw - 1) + 1)) / s->stride_w + 1;
  KGDET_CHECK_SHAPE(d.Ho >= 1 && d.Wo >= 1,
                    "Given input size: (%d x %d x %d). Calculated output size: (%d x %d x %d). Output size is too small",
                    s->C, s->H, s->W, s->O, d.Ho, d.Wo);
  d.K = s->kh * s->kw;
  d.Cg = s->C / s->groups;
  d.Og = s->O / s->groups;
  d.Cg_pad = (int)align_up(d.Cg, kChunk);
  d.Og_pad = (int)align_up(d.Og, kTileM);
  d.Og_pad16 = (int)align_up(d.Og, kChunk);
  d.Cg_pad256 = (int)align_up(d.Cg, kTileM);
  const long long in_bytes = 4LL * s->N * s->C * s->H * s->W;
  const long long out_bytes = 4LL * s->N * o_total(s) * d.Ho * d.Wo;
  const long long off_bytes = 4LL * s->N * s->deformable_groups * 2 * d.K * d.Ho * d.Wo;
  KGDET_CHECK_SHAPE(in_bytes < (1LL << 31) && out_bytes < (1LL << 31) && off_bytes < (1LL << 31),
                    "tensor larger than 2 GiB is not supported");
  return KGDET_OK;
}

// same sampling positions for the same offsets: batch, map, kernel, stride, padding, dilation (and, where the caller's
// records hold every deformable group, their number)
bool same_geometry(const kgdet_dcn_shape *a, const kgdet_dcn_shape *b, bool and_deformable_groups) {
  return a->N == b->N && a->H == b->H && a->W == b->W && a->kh == b->kh && a->kw == b->kw &&
         a->stride_h == b->stride_h && a->stride_w == b->stride_w && a->pad_h == b->pad_h && a->pad_w == b->pad_w &&
         a->dil_h == b->dil_h && a->dil_w == b->dil_w &&
         (!and_deformable_groups || a->deformable_groups == b->deformable_groups);
}

// Where the four images of weight group g sit inside a packed weight (offsets in floats):
// [forward image per group ...][transposed (backward-input) image per group ...]
// ... [bf16 hi/lo image of the plane forward kernel per group ...][its transpose per group ...]
struct WeightImages {
  size_t fwd, bwd, split, split_t;
  size_t total;   // floats of the whole packed weight
};
WeightImages weight_images(const kgdet_dcn_shape *s, const Derived &d, int g) {
  const size_t G = (size_t)s->groups;
  WeightImages w;
  w.fwd = (size_t)g * d.fwd_image_floats();
  w.bwd = G * d.fwd_image_floats() + (size_t)g * d.bwd_image_floats();
  w.split = G * (d.fwd_image_floats() + d.bwd_image_floats()) + (size_t)g * d.plane_image_floats();
  w.split_t = G * (d.fwd_image_floats() + d.bwd_image_floats() + d.plane_image_floats()) + (size_t)g * d.plane_t_image_floats();
  w.total = G * (d.fwd_image_floats() + d.bwd_image_floats() + d.plane_image_floats() + d.plane_t_image_floats());
  return w;
}
// the split (bf16 hi/lo) images depend on the WEIGHT alone (never on the map size or batch: a packed weight is reused across
// pyramid levels and batch sizes -- kgdet_amd/dcn.py caches it for inference)
bool split_images_ok(const kgdet_dcn_shape *s) {
  const int cpdg = s->C / s->deformable_groups;
  return (cpdg % 4 == 0 || s->deformable_groups == 1) && (s->deformable_groups == 1 || cpdg % 16 == 0);
}

int grid_size() {
  const int cus = cu_count();
  return cus > 0 ? cus : 256;
}

constexpr int kSlabSlots = 8;  // partial tiles a workgroup may write per launch (plane kernel: one per range it meets)
size_t slab_bytes() { return (size_t)grid_size() * kSlabSlots * kTileElems * sizeof(float); }

// A stream-K workgroup writes one slab per range its slice meets.  `units` stages dealt to G workgroups, ranges no shorter
// than min_len stages: does the slice of one workgroup stay within kSlabSlots ranges?  (Large N / many M tiles / a device
// with few CUs: beyond the bound the slab index would run into the next workgroup's slabs.)
bool slab_slots_fit(long long units, int G, int min_len) {
  const long long share = (units + G - 1) / G;
  return (share + min_len - 1) / min_len + 2 <= kSlabSlots;
}
// (the share of a workgroup up to which the rule holds whatever the total)
long long slab_slots_max_share(int min_len) { return (long long)(kSlabSlots - 2) * min_len; }
// one problem alone in a launch on the full grid: `tiles` tiles of `cpt` stages each
bool slab_slots_ok(long long tiles, int cpt) { return slab_slots_fit(tiles * cpt, grid_size(), cpt); }
int group_min_len(const DcnFwdGroup &grp) {   // shortest range (stages) of the group
  int min_len = 1 << 30;
  for (int i = 0; i < grp.n; ++i) min_len = std::min(min_len, grp.p[i].chunks_per_tile);
  return min_len;
}

// LDS-privatised backward-input: one (image, 32-channel slice) plane set must fit in LDS
struct BwdLdsPlan {
  bool ok;
  int n_cslices, S, n_blocks, n_pblocks, n_slices_total, HWp;
  size_t lds_bytes, slab_floats, off_floats, mask_floats, rowptr_ints, entry_pairs, index_lds_bytes;
  size_t workspace_bytes() const {
    return (slab_floats + off_floats + mask_floats) * sizeof(float) + rowptr_ints * sizeof(int) + entry_pairs * 8 + 64;
  }
};

BwdLdsPlan plan_bwd_lds(const kgdet_dcn_shape *s, const Derived &d) {
  BwdLdsPlan pl{};
  pl.HWp = (int)align_up((size_t)d.Ho * d.Wo, 64);
  pl.lds_bytes = (size_t)32 * pl.HWp * sizeof(float) + 8 * 256 * 8;  // colgrad tile [32][HWp] + 8 entry windows
  const int cpdg = s->C / s->deformable_groups;
  // a 32-channel slice must not straddle deformable groups
  const bool dg_ok = s->deformable_groups == 1 || cpdg % d.Cg == 0 || (d.Cg % cpdg == 0 && cpdg % 32 == 0);
  pl.index_lds_bytes = ((size_t)2 * s->H * s->W + 2) * sizeof(int) + (size_t)4 * d.Ho * d.Wo * 8;
  pl.ok = pl.lds_bytes <= kMaxLds && pl.index_lds_bytes <= kMaxLds - 64 && s->H * s->W <= 17 * 64 && dg_ok;
  pl.n_cslices = ceil_div(d.Cg, 32);
  const int pairs = s->N * pl.n_cslices;
  pl.S = grid_size() / pairs;
  if (pl.S < 1) pl.S = 1;
  if (pl.S > 64) pl.S = 64;
  pl.n_blocks = pairs * pl.S;
  pl.n_pblocks = ceil_div(d.Ho * d.Wo, 64);
  pl.n_slices_total = s->groups * pl.n_cslices;
  pl.slab_floats = (size_t)pl.n_blocks * 32 * s->H * s->W;
  pl.off_floats = (size_t)pl.n_slices_total * s->N * 2 * d.K * d.Ho * d.Wo;
  pl.mask_floats = pl.off_floats / 2;
  pl.rowptr_ints = (size_t)s->N * s->deformable_groups * d.K * ((size_t)s->H * s->W + 1);
  pl.entry_pairs = (size_t)s->N * s->deformable_groups * d.K * 4 * d.Ho * d.Wo;
  return pl;
}

// the MFMA kernels gather 4 consecutive channels per thread with one Tap, so a deformable group
// boundary must not fall inside such a quad
bool mfma_ok(const kgdet_dcn_shape *s) {
  return s->W >= 2 && ((s->C / s->deformable_groups) % 4 == 0 || s->deformable_groups == 1);
}
// the fused weight packer and every split-operand kernel stage 8 x 33 rows of K + 1 floats
bool pack_lds_ok(const Derived &d) { return (size_t)8 * 33 * (d.K + 1) * sizeof(float) <= kMaxLds - 64; }
// the forward of one problem alone on the full grid, split-operand kernels
bool fwd_slots_ok(const kgdet_dcn_shape *s, const Derived &d) {
  return slab_slots_ok((long long)s->N * ceil_div(d.Ho * d.Wo, kTileN) * (d.Og_pad / kTileM), d.K * (d.Cg_pad / kChunk));
}
// plane forward kernel: a 16-channel slice of one input image must fit in LDS next to the operand stages
bool plane_ok(const kgdet_dcn_shape *s, const Derived &d) {
  const int cpdg = s->C / s->deformable_groups;  // a producer thread samples a 16-channel chunk with one tap record
  return mfma_ok(s) && (s->deformable_groups == 1 || cpdg % 16 == 0) && s->H * s->W <= kPlaneMaxHW && pack_lds_ok(d) &&
         fwd_slots_ok(s, d);
}
size_t tap_records(const kgdet_dcn_shape *s, const Derived &d) {   // one per (image, deformable group, tap, output pixel)
  return (size_t)s->N * s->deformable_groups * d.K * d.Ho * d.Wo;
}
// forward on maps beyond the LDS plane: producers gather from a pixel-major copy of x (plane_role MODE 2); offsets into
// that copy and into the weight image must stay below 4 GB
bool gather_ok(const kgdet_dcn_shape *s, const Derived &d) {
  const int cpdg = s->C / s->deformable_groups;
  return mfma_ok(s) && (s->deformable_groups == 1 || cpdg % 16 == 0) && !plane_ok(s, d) &&
         s->C % 4 == 0 &&                                     // (a pixel's channel quads are 16-byte loads)
         (size_t)s->N * s->H * s->W * s->C * 4 < ((size_t)1 << 32) - 4096 &&
         tap_records(s, d) * sizeof(DcnTapRec) < ((size_t)1 << 32) && pack_lds_ok(d);
}
size_t gather_table_bytes(const kgdet_dcn_shape *s, const Derived &d) { return align_up(tap_records(s, d) * sizeof(DcnTapRec), 256); }
size_t gather_image_bytes(const kgdet_dcn_shape *s) { return align_up((size_t)s->N * s->H * s->W * s->C * 4 + 256, 256); }
size_t tap_table_bytes(const kgdet_dcn_shape *s, const Derived &d) { return plane_ok(s, d) ? tap_records(s, d) * sizeof(DcnTapRec) : 0; }
// the blocked copy of one input window (Cg_pad channels) the LDS-DMA plane hand-overs read
size_t xblk_copy_bytes(int N, int Cg_pad, int HW) { return align_up(dcn_xblk_bytes(N, Cg_pad, HW), 256); }
// forward on the plane kernel: the tap records and, behind them, the blocked input copy of every weight group
size_t fwd_table_bytes(const kgdet_dcn_shape *s, const Derived &d) {
  return tap_table_bytes(s, d) + (plane_ok(s, d) ? 512 + s->groups * xblk_copy_bytes(s->N, d.Cg_pad, s->H * s->W) : 0);
}
// grad_weight, split-operand kernels: the bf16 hi/lo grad_out image of one weight group / of the convolution
size_t gq_group_bytes(const kgdet_dcn_shape *s, const Derived &d) {
  return (size_t)(d.Og_pad / kTileM) * s->N * ceil_div(d.Ho * d.Wo, kChunk) * 16384;
}
size_t gq_image_bytes(const kgdet_dcn_shape *s, const Derived &d) { return (size_t)s->groups * gq_group_bytes(s, d); }
// grad_weight, fp32 kernel: the packed gradient image behind the slabs
size_t wgrad_image_bytes(const kgdet_dcn_shape *s, const Derived &d) { return (size_t)s->groups * d.fwd_image_floats() * sizeof(float); }

// Channel runs of the backward plane kernels: maximal runs of input channels inside one weight group AND one deformable
// group (one run = one sub-problem: its own tap / inverse records, its weight group's operand image and grad_out window).
// Returns their number and writes the first `cap` of them.  No run is longer than the first.
struct ChannelRun { int c0, c1, g, dgi; };
int channel_runs(const kgdet_dcn_shape *s, const Derived &d, ChannelRun *runs, int cap) {
  const int cpdg = s->C / s->deformable_groups;
  int n = 0;
  for (int c0 = 0; c0 < s->C;) {
    const int g = c0 / d.Cg, dgi = c0 / cpdg;
    const int c1 = std::min((g + 1) * d.Cg, (dgi + 1) * cpdg);
    if (n < cap) runs[n] = ChannelRun{c0, c1, g, dgi};
    ++n;
    c0 = c1;
  }
  return n;
}
// grad_input on the plane kernel: a 16-channel slice of one grad_output image in LDS; a channel run must start on a
// 256-row tile of the transposed weight image or end inside the tile it starts in
bool plane_bwd_input_ok(const kgdet_dcn_shape *s, const Derived &d) {
  ChannelRun runs[kMaxFwdGroup];
  const int n_runs = channel_runs(s, d, runs, kMaxFwdGroup);
  if (n_runs > kMaxFwdGroup) return false;
  for (int i = 0; i < n_runs; ++i) {
    const int row0 = (runs[i].c0 - runs[i].g * d.Cg) % kTileM;
    if (row0 != 0 && row0 + (runs[i].c1 - runs[i].c0) > kTileM) return false;
  }
  return d.Ho * d.Wo <= kPlaneMaxHW && s->H * s->W <= kPlaneMaxHW && s->W >= 1 && pack_lds_ok(d) &&
         dcn_build_inverse_taps_lds_bytes(s->H * s->W, d.Ho * d.Wo) <= kMaxLds - 64 &&
         slab_slots_ok((long long)n_runs * s->N * ceil_div(s->H * s->W, kTileN) * (d.Cg_pad256 / kTileM),
                       d.K * (d.Og_pad16 / kChunk));
}
// grad_offset on the plane kernel: <= 256 output channels per group; every deformable group inside ONE weight group (its
// sum then comes from one sub-problem; a deformable group spread over several weight groups would need a sum over them),
// in whole 16-channel chunks
bool plane_bwd_offset_ok(const kgdet_dcn_shape *s, const Derived &d, bool masked = false) {
  const int cpdg = s->C / s->deformable_groups;
  const bool runs_ok = (s->groups == 1 && s->deformable_groups == 1) ||
                       (d.Cg % cpdg == 0 && cpdg % kChunk == 0 && s->deformable_groups <= kMaxFwdGroup);
  return runs_ok && d.Og <= 256 && d.K <= 64 && s->H * s->W <= kPlaneMaxHW &&
         dcn_bwd_offset_plane_lds_bytes(2, d.K, s->H * s->W, masked) <= kMaxLds && pack_lds_ok(d) &&
         slab_slots_ok((long long)s->N * ceil_div(d.Ho * d.Wo, kTileN), d.K * (ceil_div(cpdg, kChunk)));
}
// grad_offset records (v2 records: 64 B; one table per deformable group)
size_t grad_tap_stride(const kgdet_dcn_shape *s, const Derived &d) { return (size_t)s->N * d.K * d.Ho * d.Wo * 64; }
size_t grad_tap_bytes(const kgdet_dcn_shape *s, const Derived &d) { return s->deformable_groups * grad_tap_stride(s, d); }

// The inverse-sampling tables of ONE deformable group (functions of the offsets alone), in this order:
struct InvTables {
  size_t rec_bytes, hdr_bytes, cell_bytes, spill_bytes;
  size_t hot_cols_bytes, hot_count_bytes;   // the hot cells' column list (dcn_hot_gemm)
  size_t total() const { return rec_bytes + hdr_bytes + cell_bytes + spill_bytes + hot_cols_bytes + hot_count_bytes; }
  size_t stride() const { return align_up(total(), 256); }
};
InvTables inv_tables(const kgdet_dcn_shape *s, const Derived &d) {
  InvTables t;
  const int slots = dcn_inv_max_slots(s->H * s->W, d.Ho * d.Wo);
  t.rec_bytes = (size_t)s->N * d.K * s->H * s->W * 64;
  t.hdr_bytes = align_up((size_t)s->N * d.K * sizeof(int), 64);
  t.cell_bytes = align_up((size_t)s->N * d.K * slots * sizeof(DcnInvOvfCell), 64);
  t.spill_bytes = (size_t)s->N * d.K * 4 * d.Ho * d.Wo * 8;
  t.hot_cols_bytes = align_up((size_t)s->N * kHotMaxCols * sizeof(int4), 256);
  t.hot_count_bytes = align_up((size_t)s->N * sizeof(int), 256);
  return t;
}
struct InvTablePtrs {
  uint4 *rec;
  int *hdr;
  DcnInvOvfCell *cells;
  int2 *spill;
  int4 *hot_cols;
  int *hot_count;
  InvTablePtrs(unsigned char *base, const InvTables &t) {
    rec = (uint4 *)base;
    hdr = (int *)(base += t.rec_bytes);
    cells = (DcnInvOvfCell *)(base += t.hdr_bytes);
    spill = (int2 *)(base += t.cell_bytes);
    hot_cols = (int4 *)(base += t.spill_bytes);
    hot_count = (int *)(base += t.hot_cols_bytes);
  }
};
size_t inv_tables_all(const kgdet_dcn_shape *s, const Derived &d) { return s->deformable_groups * inv_tables(s, d).stride(); }
// what depends on grad_output as well: the pre-aggregated sums of the long cells (one table per deformable group) and
// the pixel-major copy of the convolution's grad_output channels they are formed from
int inv_gov_slots(const kgdet_dcn_shape *s, const Derived &d) { return dcn_inv_max_slots(s->H * s->W, d.Ho * d.Wo); }
int inv_gov_ld(const kgdet_dcn_shape *s, const Derived &d) { return s->groups * d.Og_pad16; }
size_t inv_gov_bytes(const kgdet_dcn_shape *s, const Derived &d) {   // of ONE deformable group
  return align_up((size_t)s->N * d.K * inv_gov_slots(s, d) * inv_gov_ld(s, d) * sizeof(float), 256);
}
size_t inv_gout_t_bytes(const kgdet_dcn_shape *s, const Derived &d) { return align_up((size_t)s->N * d.Ho * d.Wo * s->O * sizeof(float), 256); }
size_t inv_sums_all(const kgdet_dcn_shape *s, const Derived &d) { return s->deformable_groups * inv_gov_bytes(s, d) + inv_gout_t_bytes(s, d); }
// grad_input on the plane kernel: everything behind the slabs
size_t bwd_input_table_bytes(const kgdet_dcn_shape *s, const Derived &d) { return inv_tables_all(s, d) + inv_sums_all(s, d); }
// backward tiles (256 / 128 channels wide) must lie inside one deformable group
bool mfma_bwd_ok(const kgdet_dcn_shape *s) {
  const int cpdg = s->C / s->deformable_groups, Cg = s->C / s->groups;
  return s->deformable_groups == 1 || cpdg % Cg == 0 || (Cg % cpdg == 0 && cpdg % kTileM == 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// Groups and (sub-)problems
// ---------------------------------------------------------------------------------------------------------------------
void fill_problem(const kgdet_dcn_shape *s, const Derived &d, int group, DcnProblem &p) {
  p = DcnProblem{};
  p.N = s->N; p.C_total = s->C; p.c_base = group * d.Cg; p.Cg = d.Cg; p.Cg_pad = d.Cg_pad;
  p.O_total = o_total(s);
  p.o_base = s->out_channel_offset + group * d.Og; p.Og = d.Og; p.Og_pad = d.Og_pad;
  p.bias_base = group * d.Og;
  p.H = s->H; p.W = s->W; p.Ho = d.Ho; p.Wo = d.Wo; p.HoWo = d.Ho * d.Wo; p.P = s->N * p.HoWo;
  p.kh = s->kh; p.kw = s->kw; p.K = d.K; p.seg_stages = d.K;
  p.sh = s->stride_h; p.sw = s->stride_w; p.ph = s->pad_h; p.pw = s->pad_w; p.dh = s->dil_h; p.dw = s->dil_w;
  p.DG = s->deformable_groups; p.cpdg = s->C / s->deformable_groups;
}

// A group without problems.  xcd = 0 with two slots is the exact-fp32 kernel's slab numbering (DcnFwdGroup::xcd_slices).
DcnFwdGroup empty_group(int slots, int gather_mode, int wave_layout, int xcd = 1) {
  DcnFwdGroup grp;
  grp.n = 0;
  grp.xcd_slices = xcd;
  grp.slots = slots;
  grp.dbl_plane = 0;
  grp.plane_bytes = 0;
  grp.wave_layout = wave_layout;
  grp.pair_mode = 0;
  grp.gather_mode = gather_mode;
  grp.rounds = 1;
  grp.static_ranges = 0;
  grp.tile_begin[0] = 0; grp.range_begin[0] = 0; grp.unit_begin[0] = 0;
  return grp;
}
// Tiles, ranges and units of a problem are n_ntiles * n_mtiles (x chunks_per_tile); a grad_offset problem has ONE row tile
// (n_mtiles = 1: its <= 256 output channels), so its counts are n_ntiles.  kparts == 1 here: plan_static_ranges may cut
// the reductions afterwards and then rewrites range_begin.
void append_problem(DcnFwdGroup &grp, const DcnProblem &p) {
  const int i = grp.n++, tiles = p.n_ntiles * p.n_mtiles;
  grp.p[i] = p;
  grp.tile_begin[i + 1] = grp.tile_begin[i] + tiles;
  grp.range_begin[i + 1] = grp.range_begin[i] + tiles;
  grp.unit_begin[i + 1] = grp.unit_begin[i] + p.total_units;
}

// Forward problem of weight group g.  per_image: pixel tiles never straddle images and the split weight image is set (plane
// and gather kernels); otherwise tiles run over N * Ho * Wo (exact-fp32 kernel).
DcnProblem forward_problem(const kgdet_dcn_shape *s, const Derived &d, int g, const float *input, const float *offset,
                           const float *mask, const float *packed_weight, const float *bias, float *output, uint32_t flags,
                           bool per_image) {
  const WeightImages wi = weight_images(s, d, g);
  DcnProblem p;
  fill_problem(s, d, g, p);
  p.x = input; p.offset = offset; p.mask = mask; p.bias = bias; p.out = output;
  p.wpk = packed_weight + wi.fwd;
  p.flags = flags;
  p.n_ntiles = ceil_div(p.P, kTileN);
  p.n_mtiles = d.Og_pad / kTileM;
  p.chunks_per_tap = d.Cg_pad / kChunk;
  p.chunks_per_tile = d.K * p.chunks_per_tap;
  if (per_image) {
    p.wq = packed_weight + wi.split;
    p.tiles_per_image = ceil_div(p.HoWo, kTileN);
    p.n_ntiles = p.N * p.tiles_per_image;
  }
  p.total_units = (long long)p.n_ntiles * p.n_mtiles * p.chunks_per_tile;
  // kparts > 1 would cut the reduction so that one part's weights fit a per-XCD L2 (units ordered problem, part,
  // tile, stage -- supported by dcn_unit_pos and the fix-up).  Measured on MI355X: no gain -- the weight stream
  // is not what bounds the kernel (an always-hot weight stage bought 6 %) -- while the extra partial tiles cost
  // 25 %; it stays 1.
  p.kparts = 1;
  return p;
}

// grad_input of one channel run, the transposed problem: "input" = grad_output window of the run's weight group,
// "output" = the run's grad_input channels.  `inv` / `gov`: the inverse records and long-cell sums of the run's
// deformable group.
DcnProblem grad_input_problem(const kgdet_dcn_shape *s, const Derived &d, const ChannelRun &run, const float *grad_output,
                              float *grad_input, const float *packed_weight, const void *inv, const float *gov) {
  const int g = run.g, len = run.c1 - run.c0, row = run.c0 - g * d.Cg;
  DcnProblem p{};
  p.x = grad_output; p.out = grad_input;
  p.N = s->N;
  p.C_total = o_total(s); p.c_base = s->out_channel_offset + g * d.Og; p.Cg = d.Og; p.Cg_pad = d.Og_pad16;
  p.O_total = s->C; p.o_base = run.c0; p.Og = len; p.Og_pad = ceil_div(len, kTileM) * kTileM; p.bias_base = 0;
  p.mt_base = row / kTileM; p.row0 = row % kTileM;
  p.H = d.Ho; p.W = d.Wo;                       // plane geometry = grad_output
  p.Ho = s->H; p.Wo = s->W; p.HoWo = s->H * s->W; p.P = s->N * p.HoWo;  // "pixels" = input cells
  p.kh = s->kh; p.kw = s->kw; p.K = d.K; p.seg_stages = d.K;
  p.DG = 1; p.cpdg = p.C_total;
  p.tiles_per_image = ceil_div(p.HoWo, kTileN);
  p.n_ntiles = p.N * p.tiles_per_image;
  p.n_mtiles = p.Og_pad / kTileM;
  p.chunks_per_tap = d.Og_pad16 / kChunk;
  p.chunks_per_tile = d.K * p.chunks_per_tap;
  p.total_units = (long long)p.n_ntiles * p.n_mtiles * p.chunks_per_tile;
  p.kparts = 1;
  p.flags = 0;
  p.wq = packed_weight + weight_images(s, d, g).split_t;
  p.taps = reinterpret_cast<const DcnTapRec *>(inv);
  p.inv_gov = gov;
  p.gov_slots = inv_gov_slots(s, d); p.gov_ld = inv_gov_ld(s, d); p.gov_c0 = g * d.Og_pad16;
  p.build_taps = 0;
  return p;
}

// grad_offset (v1: mask == nullptr; v2: mask and grad_mask) of one channel run = one deformable group
// (plane_bwd_offset_ok), with the record table `taps`.
DcnProblem grad_offset_problem(const kgdet_dcn_shape *s, const Derived &d, const ChannelRun &run, const float *input,
                               const float *offset, const float *mask, const float *packed_weight, const float *grad_output,
                               float *grad_offset, float *grad_mask, const void *taps, bool build_taps, uint32_t flags) {
  const int g = run.g;
  DcnProblem p;
  fill_problem(s, d, g, p);
  p.x = input; p.offset = offset; p.mask = mask; p.gout = grad_output; p.goff = grad_offset; p.gmask = grad_mask;
  p.c_base = run.c0; p.Cg = run.c1 - run.c0; p.Cg_pad = ceil_div(p.Cg, kChunk) * kChunk;
  p.dgi = run.dgi; p.c16_base = (run.c0 - g * d.Cg) / kChunk;
  p.wq = packed_weight + weight_images(s, d, g).split_t;
  p.taps = reinterpret_cast<const DcnTapRec *>(taps); p.build_taps = build_taps;
  p.tiles_per_image = ceil_div(p.HoWo, kTileN);
  p.n_ntiles = p.N * p.tiles_per_image;
  p.n_mtiles = 1;
  p.chunks_per_tap = p.Cg_pad / kChunk;
  p.chunks_per_tile = d.K * p.chunks_per_tap;
  p.total_units = (long long)p.n_ntiles * p.chunks_per_tile;
  p.kparts = 1;
  p.flags = flags;
  return p;
}

// grad_weight of one channel run: rows = the weight group's output channels (its grad_out image `gq`), columns =
// (16-channel chunk of the run, group of `taps_per_tile` taps), reduction over the pixels of all images.
DcnProblem grad_weight_problem(const kgdet_dcn_shape *s, const Derived &d, const ChannelRun &run, const float *input,
                               const float *offset, const float *mask, float *grad_weight, const void *taps, bool build_taps,
                               const void *gq, int taps_per_tile) {
  const int g = run.g, n_px16 = ceil_div(d.Ho * d.Wo, kChunk);
  DcnProblem p;
  fill_problem(s, d, g, p);
  p.x = input; p.offset = offset; p.mask = mask;
  p.c_base = run.c0; p.Cg = run.c1 - run.c0; p.Cg_pad = ceil_div(p.Cg, kChunk) * kChunk;
  p.dgi = run.dgi;
  p.w_ld = d.Cg;                                                      // a weight row holds the whole group's channels
  p.out = grad_weight + ((size_t)g * d.Og * d.Cg + (size_t)(run.c0 - g * d.Cg)) * d.K;
  p.taps = reinterpret_cast<const DcnTapRec *>(taps);
  p.build_taps = build_taps;
  p.wq = gq;
  p.n_mtiles = d.Og_pad / kTileM;
  p.tiles_per_image = ceil_div(d.K, taps_per_tile);        // tap groups per channel chunk
  p.n_ntiles = (p.Cg_pad / kChunk) * p.tiles_per_image;    // (chunk, tap group) column tiles
  p.chunks_per_tap = n_px16;                               // stages per image
  p.chunks_per_tile = s->N * n_px16;                       // the reduction runs over the pixels of all images
  p.total_units = (long long)p.n_ntiles * p.n_mtiles * p.chunks_per_tile;
  p.kparts = 1;
  p.flags = 0;
  return p;
}

// plane kernels (forward / grad_input): LDS of the launch = the largest need over the group's problems.
// (A second plane buffer, filled by the producer waves while the current chunk runs, was measured and dropped: the
// launch got slower, 256 -> 271 us at B=2 and 598 -> 686 us at B=8 -- the producers are the critical path of a stage
// and the copy adds to exactly their work, while the synchronous copy by all twelve waves is ~6 % of a workgroup.)
size_t plan_plane_lds(DcnFwdGroup &grp, size_t single, size_t fixed) {
  grp.plane_bytes = (int)(single - fixed);
  return single;
}

// Static split-K for the plane kernels (forward / grad_input): cut every problem's reduction into parts of about one
// workgroup's share (whole channel chunks) so that the (problem, part, tile) ranges can be dealt ONE per workgroup.
// Ranges of one (problem, part) are consecutive and consecutive slices sit on one XCD (sk_slice_of_block), so the
// workgroups of an XCD stream the same weight stages at the same time: L2 hits instead of one fabric read per pixel
// tile.  Measured on the head-stage forward (6 problems, B=2): fabric reads 883 -> 174 MB per launch, 265 -> 207 us.
// Falls back to stream-K (static_ranges = 0, kparts = 1) when the ranges outnumber the workgroups or would be too
// uneven.  Problems must have kparts == 1 on entry.
// max_rounds > 1 (forward / grad_input plane kernels): when a workgroup's share is long (B = 8 inference: 747 stages) the
// ranges are cut to ~190 stages all the same and dealt in ROUNDS -- workgroup r computes ranges r, r + G, ... -- instead
// of falling back to stream-K: every range still starts on a channel chunk, the tiles of one (problem, part) still run
// together on one XCD, and the fix-up stays the cheap static one.
void plan_static_ranges(DcnFwdGroup &grp, int G, bool force = false, int max_rounds = 1) {
  grp.static_ranges = 0;
  grp.rounds = 1;
  const long long total = grp.unit_begin[grp.n];
  static const int env_rounds = env_int("KGDET_DCN_ROUNDS", 0);   // A/B switch
  if (env_rounds > 0 && max_rounds > 1) max_rounds = env_rounds;
  int R = (int)((double)total / G / 220.0 + 0.999);
  R = R < 1 ? 1 : (R > max_rounds ? max_rounds : R);
  const double share = (double)total / G / R;   // target length of a range
  int ranges = 0;
  double longest = 0;
  int kp[kMaxFwdGroup];
  for (int i = 0; i < grp.n; ++i) {
    const DcnProblem &q = grp.p[i];
    int k = (int)((double)q.chunks_per_tile / share + 0.5);
    k = k < 1 ? 1 : (k > q.chunks_per_tap ? q.chunks_per_tap : k);
    kp[i] = k;
    ranges += q.n_ntiles * q.n_mtiles * k;
    const double len = (double)((q.chunks_per_tap + k - 1) / k) * q.seg_stages;
    longest = len > longest ? len : longest;
  }
  static const bool off = env_present("KGDET_DCN_STREAMK");   // A/B switch
  if (force) {   // a kernel without a stream-K fix-up (v2 grad_offset): fewer, longer parts until the ranges fit
    R = 1;
    while (ranges > G) {
      int worst = 0;
      for (int i = 1; i < grp.n; ++i)
        if (kp[i] > kp[worst]) worst = i;
      if (kp[worst] == 1) return;   // more tiles than workgroups: no static schedule
      ranges -= grp.p[worst].n_ntiles * grp.p[worst].n_mtiles * (kp[worst] - (kp[worst] + 1) / 2);
      kp[worst] = (kp[worst] + 1) / 2;
    }
  } else if (off || ranges > R * G || longest > 1.25 * share) {
    return;
  }
  grp.static_ranges = 1;
  grp.rounds = (ranges + G - 1) / G;
  for (int i = 0; i < grp.n; ++i) {
    grp.p[i].kparts = kp[i];
    grp.range_begin[i + 1] = grp.range_begin[i] + grp.p[i].n_ntiles * grp.p[i].n_mtiles * kp[i];
  }
}

// fix-up launch of a plane-kernel group: the static schedule has its own, cheaper kernel
void launch_plane_fixup(const DcnFwdGroup &grp, const void *workspace, int G, void *stream) {
  if (grp.static_ranges)
    hipLaunchKernelGGL(dcn_fwd_fixup_static, dim3(grp.tile_begin[grp.n], 2), dim3(kThreads), 0, (hipStream_t)stream, grp,
                       (const float *)workspace, G);
  else
    hipLaunchKernelGGL(dcn_fwd_fixup, dim3(grp.tile_begin[grp.n], 16), dim3(kThreads), 0, (hipStream_t)stream, grp,
                       (const float *)workspace, G);
}

// Grid of a plane-kernel launch: small groups run on fewer workgroups, so that a workgroup's share is at least ~16 stages.
// (With all 256 workgroups on the 7 x 11 level of a five-level head -- 2 tiles x 144 stages -- every workgroup computed one stage
// and wrote a 128 KB slab; the fix-up then added 128 slabs per tile with two workgroups: 128 us per launch, four launches per step.)
int small_launch_grid(const DcnFwdGroup &grp, int G) {
  static const bool off = env_present("KGDET_DCN_FULL_GRID");   // A/B switch
  // (a slice must not meet more ranges than it has slab slots)
  const long long per = std::max<long long>(1, std::min<long long>(16, slab_slots_max_share(group_min_len(grp))));
  const long long g = grp.unit_begin[grp.n] / per;
  return off ? G : (int)std::max<long long>(1, std::min<long long>(G, g));
}

// Sum groups of a backward launch (DcnProblem::sum_count): problems whose OUTPUT POINTERS coincide are summed into that one tensor
// by the fix-up.  Members must tile alike (same images, pixels, rows); at most four per group.  Returns false otherwise.
bool assign_sum_groups(DcnFwdGroup &grp, const void *const *outs, bool same_taps) {
  for (int i = 0; i < grp.n; ++i) { grp.p[i].sum_count = 0; }
  for (int i = 0; i < grp.n; ++i) {
    int lead = i;
    for (int j = 0; j < i; ++j)
      if (outs[j] == outs[i]) { lead = j; break; }
    if (lead == i) continue;
    DcnProblem &L = grp.p[lead];
    const DcnProblem &q = grp.p[i];
    if (L.sum_count == 0) { L.sum_count = 1; L.sum_members[0] = lead; }
    if (L.sum_count >= 4 || q.N != L.N || q.HoWo != L.HoWo || q.Og != L.Og || q.n_ntiles != L.n_ntiles || q.n_mtiles != L.n_mtiles ||
        q.tiles_per_image != L.tiles_per_image || (same_taps && q.K != L.K))
      return false;
    L.sum_members[L.sum_count++] = i;
  }
  for (int i = 0; i < grp.n; ++i) {        // every member carries the group (the kernels test sum_count, the fix-up the leader)
    const DcnProblem &L = grp.p[i];
    if (L.sum_count > 1 && L.sum_members[0] == i)
      for (int m = 1; m < L.sum_count; ++m) {
        DcnProblem &q = grp.p[L.sum_members[m]];
        q.sum_count = L.sum_count;
        for (int e = 0; e < 4; ++e) q.sum_members[e] = L.sum_members[e];
      }
  }
  return true;
}
bool has_sum_groups(const DcnFwdGroup &grp) {
  for (int i = 0; i < grp.n; ++i)
    if (grp.p[i].sum_count > 1) return true;
  return false;
}
// grad_offset on tap pairs (dcn_backward_offset_pair.hip): v1, split operands, one static range per workgroup, K >= 3 (a tap's
// running sum is re-read one segment later, one slot ahead of its use: with a single pair per segment that would be the slot it is
// written in)
bool offset_pair_ok(const DcnFwdGroup &grp) {
  static const bool off = env_int("KGDET_DCN_OFFSET_PAIR", 1) == 0;   // A/B switch
  if (off || !grp.static_ranges || grp.rounds != 1) return false;
  for (int i = 0; i < grp.n; ++i) {
    const DcnProblem &q = grp.p[i];
    if (q.mask || q.K < 3 || q.Og > 256 || q.Og % 32 != 0 || q.H * q.W > kPlaneMaxHW) return false;   // (Og % 32: a DMA piece = two 16-o chunks)
  }
  return true;
}
// Blocked copies of the distinct inputs of a group behind its record tables (`used` of `table_cap` bytes behind the slabs taken;
// written by the record builder's blocks), shared by the problems that read the same window.  No room for one: must_fit returns
// KGDET_E_WORKSPACE (forward); otherwise that problem goes without and its plane switches copy through registers (grad_offset).
int place_xblk(DcnFwdGroup &grp, bool enabled, unsigned char *table_base, size_t used, size_t table_cap, bool must_fit) {
  used = align_up(used, 256);
  for (int i = 0; i < grp.n; ++i) {
    DcnProblem &q = grp.p[i];
    q.xblk = nullptr; q.build_xblk = 0;
    if (!enabled) continue;
    for (int j = 0; j < i && !q.xblk; ++j) {
      const DcnProblem &o = grp.p[j];
      if (o.xblk && o.x == q.x && o.c_base == q.c_base && o.Cg == q.Cg && o.N == q.N && o.H == q.H && o.W == q.W && o.C_total == q.C_total)
        q.xblk = o.xblk;
    }
    if (q.xblk) continue;
    const size_t xb = xblk_copy_bytes(q.N, q.Cg_pad, q.H * q.W);
    if (used + xb > table_cap) {
      if (!must_fit) continue;
      set_error("workspace too small for the blocked inputs: need %zu bytes, got %zu (kgdet_dcn_group_workspace_bytes)",
                slab_bytes() + used + xb, slab_bytes() + table_cap);
      return KGDET_E_WORKSPACE;
    }
    q.xblk = reinterpret_cast<const float *>(table_base + used);
    q.build_xblk = 1;
    used += xb;
  }
  return KGDET_OK;
}
void place_offset_xblk(DcnFwdGroup &grp, unsigned char *table_base, size_t used, size_t table_cap) {
  static const bool off = env_int("KGDET_DCN_OFFSET_XBLK", 1) == 0;   // A/B switch
  place_xblk(grp, !off, table_base, used, table_cap, false);
}
// test hook (kgdet_debug_dcn_offset_handover): how the last grad_offset launch of the process handed its planes over -- -1: not on the
// tap-pair kernel; otherwise the number of its problems that read a blocked input copy (0: every plane switch through registers)
int g_offset_handover = -1;
void note_offset_handover(const DcnFwdGroup &grp, bool use_pair) {
  g_offset_handover = -1;
  if (!use_pair) return;
  g_offset_handover = 0;
  for (int i = 0; i < grp.n; ++i) g_offset_handover += grp.p[i].xblk != nullptr;
}
int launch_offset_pair(const DcnFwdGroup &grp, int G, void *workspace, int max_K, void *stream) {
  if (int rc = allow_lds<dcn_bwd_offset_pair>(kMaxLds)) return rc;
  hipLaunchKernelGGL(dcn_bwd_offset_pair, dim3(G), dim3(dcn_bwd_offset_pair_threads()), dcn_bwd_offset_pair_lds_bytes(),
                     (hipStream_t)stream, grp, (float *)workspace, max_K);
  return KGDET_OK;
}
// the convolution's window of grad_output as a pixel-major copy [N][HoWo][O] at `gout_t`
DcnPixelMajorItem gout_pixel_major(const kgdet_dcn_shape *s, const Derived &d, const float *grad_output, float *gout_t) {
  return DcnPixelMajorItem{grad_output + (size_t)s->out_channel_offset * d.Ho * d.Wo, gout_t, s->N, s->O, d.Ho * d.Wo,
                           (long long)o_total(s) * d.Ho * d.Wo};
}
int launch_bias_grad(const kgdet_dcn_shape *s, const Derived &d, const float *grad_output, float *grad_bias, int accumulate,
                     void *stream) {
  if (!grad_bias) return KGDET_OK;
  hipLaunchKernelGGL(dcn_bias_grad, dim3(s->O), dim3(256), 0, (hipStream_t)stream,
                     grad_output + (size_t)s->out_channel_offset * d.Ho * d.Wo, grad_bias, s->N, o_total(s), d.Ho * d.Wo,
                     accumulate);
  KGDET_CHECK_LAUNCH("dcn_bias_grad");
  return KGDET_OK;
}

}  // namespace

}  // namespace kgdet

using namespace kgdet;

extern "C" {

// ---------------------------------------------------------------------------------------------------------------------
// Size queries
// ---------------------------------------------------------------------------------------------------------------------
int kgdet_dcn_output_size(const kgdet_dcn_shape *s, int32_t *Ho, int32_t *Wo) {
  Derived d;
  if (int rc = derive(s, d)) return rc;
  if (Ho) *Ho = d.Ho;
  if (Wo) *Wo = d.Wo;
  return KGDET_OK;
}

size_t kgdet_dcn_packed_weight_bytes(const kgdet_dcn_shape *s) {
  Derived d;
  if (derive(s, d)) return 0;
  return weight_images(s, d, 0).total * sizeof(float);
}

size_t kgdet_dcn_workspace_bytes(const kgdet_dcn_shape *s) {
  Derived d;
  if (derive(s, d)) return 0;
  // slabs for stream-K partial tiles + (forward) the tap records and blocked input copies / (backward-weight) a packed
  // gradient image
  size_t need = slab_bytes() + std::max(wgrad_image_bytes(s, d), fwd_table_bytes(s, d));
  const BwdLdsPlan pl = plan_bwd_lds(s, d);
  if (pl.ok) need = std::max(need, pl.workspace_bytes());
  if (plane_bwd_input_ok(s, d)) need = std::max(need, slab_bytes() + bwd_input_table_bytes(s, d));
  if (plane_bwd_offset_ok(s, d))
    need = std::max(need, slab_bytes() + align_up(grad_tap_bytes(s, d), 256) +
                              s->deformable_groups * xblk_copy_bytes(s->N, d.Cg_pad, s->H * s->W));
  if (plane_ok(s, d))   // grad_weight on the plane kernel: records + one grad_out image per weight group
    need = std::max(need, slab_bytes() + align_up(tap_table_bytes(s, d), 256) + gq_image_bytes(s, d));
  if (gather_ok(s, d))   // forward / grad_weight on large maps: records (+ grad_out images) + the pixel-major copy of x
    need = std::max(need, slab_bytes() + gather_table_bytes(s, d) + gather_image_bytes(s) + gq_image_bytes(s, d));
  if (!(pl.ok && mfma_bwd_ok(s)) || !plane_bwd_input_ok(s, d)) {   // the materialised column gradient of dcn_backward_large.hip, per channel run
    ChannelRun longest;
    channel_runs(s, d, &longest, 1);
    DcnProblem p;
    fill_problem(s, d, 0, p);
    p.C_total = longest.c1 - longest.c0;
    if (dcn_bwd_large_ok(p, false, 1)) need = std::max(need, dcn_bwd_large_workspace_bytes(p));
  }
  return need;
}

size_t kgdet_dcn_group_workspace_bytes(int32_t n, const kgdet_dcn_shape *const *shapes) {
  size_t tables = 0, bwd_tables = 0, wgrad_tables = 0, off_tables = 0, single = 0;
  for (int i = 0; i < n; ++i) {
    Derived d;
    if (!shapes || derive(shapes[i], d)) return 0;
    const kgdet_dcn_shape *s = shapes[i];
    tables += fwd_table_bytes(s, d);
    if (plane_bwd_input_ok(s, d)) bwd_tables += bwd_input_table_bytes(s, d);
    if (plane_bwd_offset_ok(s, d))   // (grad_offset phase: records + the blocked copy of the input of the tap-pair kernel)
      off_tables += align_up(grad_tap_bytes(s, d), 256) + xblk_copy_bytes(s->N, d.Cg_pad, s->H * s->W) + 256;
    wgrad_tables += align_up(tap_table_bytes(s, d), 256) + gq_image_bytes(s, d);
    single = std::max(single, kgdet_dcn_workspace_bytes(s));
  }
  // (the backward phases and grad_weight run one after the other)
  return std::max(single, slab_bytes() + std::max({tables, bwd_tables, wgrad_tables, off_tables}));
}

// 1 when EVERY product of a convolution of this shape -- forward, grad_input, grad_offset, grad_weight -- has a split-operand
// kernel: such a convolution never reads the two fp32 images of its packed weight
int32_t kgdet_dcn_split_path_complete(const kgdet_dcn_shape *s) {
  Derived d;
  if (!s || derive(s, d)) return 0;
  return s->groups == 1 && s->deformable_groups == 1 && plane_ok(s, d) && plane_bwd_input_ok(s, d) && plane_bwd_offset_ok(s, d)
             ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight packers
// ---------------------------------------------------------------------------------------------------------------------
int kgdet_dcn_pack_weight(const kgdet_dcn_shape *s, const float *weight, float *packed, void *stream) {
  Derived d;
  if (int rc = derive(s, d)) return rc;
  KGDET_CHECK_SHAPE(weight && packed, "null pointer");
  const size_t lds_all = (size_t)8 * 33 * (d.K + 1) * sizeof(float);
  const bool fused = pack_lds_ok(d);
  const size_t lds = (size_t)64 * (d.K + 1) * sizeof(float);
  KGDET_CHECK_SHAPE(fused || lds <= 64 * 1024, "kernel %dx%d too large to pack", s->kh, s->kw);
  if (fused)
    if (int rc = allow_lds<dcn_pack_weight_all>(kMaxLds - 64)) return rc;
  for (int g = 0; g < s->groups; ++g) {
    const float *w = weight + (size_t)g * d.Og * d.Cg * d.K;
    const WeightImages wi = weight_images(s, d, g);
    if (fused) {
      dim3 grid(d.Cg_pad256 / 8, d.Og_pad / 32);
      const bool split = split_images_ok(s);
      hipLaunchKernelGGL(dcn_pack_weight_all, grid, dim3(256), lds_all, (hipStream_t)stream, w, packed + wi.fwd, packed + wi.bwd,
                         split ? (void *)(packed + wi.split) : nullptr, split ? (void *)(packed + wi.split_t) : nullptr, d.Og,
                         d.Cg, d.K, d.Cg_pad, d.Og_pad, d.Og_pad16, d.Cg_pad256);
    } else {
      dim3 grid(d.Cg_pad, d.Og_pad / 64);
      hipLaunchKernelGGL(dcn_pack_weight, grid, dim3(256), lds, (hipStream_t)stream, w, packed + wi.fwd, d.Og, d.Cg, d.K,
                         d.Cg_pad, d.Og_pad);
      dim3 grid_t(d.Og_pad16, d.Cg_pad256 / 64);
      hipLaunchKernelGGL(dcn_pack_weight_t, grid_t, dim3(256), lds, (hipStream_t)stream, w, packed + wi.bwd, d.Og, d.Cg, d.K,
                         d.Og_pad16, d.Cg_pad256);
    }
  }
  KGDET_CHECK_LAUNCH("dcn_pack_weight");
  return KGDET_OK;
}

// n weights in ONE launch (every weight: one weight group, fused pack kernel); anything else: one call each
int kgdet_dcn_pack_weight_multi(int32_t n, const kgdet_dcn_shape *const *shapes, const float *const *weights,
                                float *const *packeds, void *stream) {
  return kgdet_dcn_pack_weight_images(n, shapes, weights, packeds, 3, stream);
}

int kgdet_dcn_pack_weight_images(int32_t n, const kgdet_dcn_shape *const *shapes, const float *const *weights,
                                 float *const *packeds, uint32_t images, void *stream) {
  KGDET_CHECK_SHAPE(n >= 1 && shapes && weights && packeds, "null pointer");
  KGDET_CHECK_SHAPE((images & 3u) != 0 && (images & ~3u) == 0, "images: bit 0 = the fp32 images, bit 1 = the split (bf16 hi/lo) images");
  int i = 0;
  while (i < n) {
    DcnPackGroup grp;
    int m = 0, gx = 0, gy = 0;
    size_t lds = 0;
    for (; i < n && m < kMaxFwdGroup; ++i) {
      const kgdet_dcn_shape *s = shapes[i];
      Derived d;
      if (int rc = derive(s, d)) return rc;
      KGDET_CHECK_SHAPE(weights[i] && packeds[i], "null pointer (weight %d)", i);
      if (s->groups != 1 || !pack_lds_ok(d)) {   // not the fused single-group case: on its own (all images)
        if (m > 0) break;
        if (int rc = kgdet_dcn_pack_weight(s, weights[i], packeds[i], stream)) return rc;
        continue;
      }
      const bool split = split_images_ok(s) && (images & 2u);
      // (a weight without split images keeps its fp32 ones whatever the mask says: nothing else could serve it)
      const bool fp32_images = (images & 1u) || !split;
      const WeightImages wi = weight_images(s, d, 0);
      DcnPackOne &e = grp.e[m++];
      float *packed = packeds[i];
      e.w = weights[i];
      e.wpk = fp32_images ? packed + wi.fwd : nullptr;
      e.wpt = fp32_images ? packed + wi.bwd : nullptr;
      e.wq = split ? (void *)(packed + wi.split) : nullptr;
      e.wqt = split ? (void *)(packed + wi.split_t) : nullptr;
      e.Og = d.Og; e.Cg = d.Cg; e.K = d.K; e.Cg_pad = d.Cg_pad; e.Og_pad = d.Og_pad; e.Og_pad16 = d.Og_pad16;
      e.Cg_pad256 = d.Cg_pad256;
      gx = std::max(gx, d.Cg_pad256 / 8);
      gy = std::max(gy, d.Og_pad / 32);
      lds = std::max(lds, (size_t)8 * 33 * (d.K + 1) * sizeof(float));
    }
    if (m > 0) {
      if (int rc = allow_lds<dcn_pack_weight_all_multi>(kMaxLds - 64)) return rc;
      hipLaunchKernelGGL(dcn_pack_weight_all_multi, dim3(gx, gy, m), dim3(256), lds, (hipStream_t)stream, grp);
      KGDET_CHECK_LAUNCH("dcn_pack_weight_all_multi");
    }
  }
  return KGDET_OK;
}


int kgdet_dcn_unpack_weight_grad(const kgdet_dcn_shape *s, const float *packed, float *grad_weight,
                                 int accumulate, void *stream) {
  Derived d;
  if (int rc = derive(s, d)) return rc;
  KGDET_CHECK_SHAPE(grad_weight && packed, "null pointer");
  const size_t lds = (size_t)64 * (d.K + 1) * sizeof(float);
  KGDET_CHECK_SHAPE(lds <= 64 * 1024, "kernel %dx%d too large to unpack", s->kh, s->kw);
  for (int g = 0; g < s->groups; ++g) {
    float *w = grad_weight + (size_t)g * d.Og * d.Cg * d.K;
    const float *src = packed + weight_images(s, d, g).fwd;
    dim3 grid(d.Cg, d.Og_pad / 64);
    hipLaunchKernelGGL(dcn_unpack_weight, grid, dim3(256), lds, (hipStream_t)stream, src, w, d.Og, d.Cg, d.K,
                       d.Cg_pad, d.Og_pad, accumulate);
  }
  KGDET_CHECK_LAUNCH("dcn_unpack_weight");
  return KGDET_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------------------------------------------------
int kgdet_deform_conv_forward_grouped(int32_t n, const kgdet_dcn_shape *const *shapes, const float *const *inputs,
                                      const float *const *offsets, const float *const *masks,
                                      const float *const *packed_weights, const float *const *biases,
                                      float *const *outputs, uint32_t flags, void *workspace,
                                      size_t workspace_bytes, void *stream) {
  KGDET_CHECK_SHAPE(n >= 1 && shapes && inputs && offsets && packed_weights && outputs, "null pointer / empty group");
  if (workspace_bytes < slab_bytes() || workspace == nullptr) {
    set_error("workspace too small: need %zu bytes, got %zu", slab_bytes(), workspace_bytes);
    return KGDET_E_WORKSPACE;
  }
  const int G = grid_size();
  DcnFwdGroup grp = empty_group(kSlabSlots, 0, dcn_plane_wave_layout());  // problems collected for one launch of the plane kernel
  const kgdet_dcn_shape *grp_shape[kMaxFwdGroup];                          // (their shapes)
  size_t lds = 0;
  unsigned char *const table_base = (unsigned char *)workspace + slab_bytes();
  const size_t table_cap = workspace_bytes - slab_bytes();
  size_t table_used = 0;  // bytes of tap records placed behind the slabs for the pending group
  const int parts = (flags & KGDET_DCN_BF16) ? 1 : 2;
  auto flush = [&]() -> int {
    if (grp.n == 0) return KGDET_OK;
    const int Gf = G;                                  // (the full grid: record builders)
    const int G = small_launch_grid(grp, Gf);
    plan_static_ranges(grp, G, false, kSlabSlots - 2);
    if (int rc = allow_lds<dcn_fwd_plane<1>, dcn_fwd_plane<2>>(kMaxLds)) return rc;
    static const int chain_dma = env_int("KGDET_DCN_CHAIN_DMA", 1);   // A/B switch
    // (plane kernel: chained segment hand-over by LDS-DMA from blocked copies of the inputs, written by dcn_build_taps' blocks)
    if (int rc = place_xblk(grp, chain_dma && parts == 2, table_base, table_used, table_cap, true)) return rc;
    hipLaunchKernelGGL(dcn_build_taps, dim3(2 * Gf, grp.n), dim3(256), 0, (hipStream_t)stream, grp);
    const size_t lds2 = plan_plane_lds(grp, lds, dcn_fwd_plane_fixed_lds_bytes(parts));
    if (parts == 1)
      hipLaunchKernelGGL(dcn_fwd_plane<1>, dim3(G), dim3(dcn_fwd_plane_threads()), lds2, (hipStream_t)stream, grp, (float *)workspace);
    else
      hipLaunchKernelGGL(dcn_fwd_plane<2>, dim3(G), dim3(dcn_fwd_plane_threads()), lds2, (hipStream_t)stream, grp, (float *)workspace);
    launch_plane_fixup(grp, workspace, G, stream);
    grp.n = 0;
    lds = 0;
    table_used = 0;
    return KGDET_OK;
  };
  for (int i = 0; i < n; ++i) {
    const kgdet_dcn_shape *s = shapes[i];
    Derived d;
    if (int rc = derive(s, d)) return rc;
    KGDET_CHECK_SHAPE(inputs[i] && offsets[i] && packed_weights[i] && outputs[i], "null pointer (problem %d)", i);
    if (!mfma_ok(s)) {
      set_error("deformable_groups=%d with %d channels per group is not supported by the MFMA path",
                s->deformable_groups, s->C / s->deformable_groups);
      return KGDET_E_UNSUPPORTED;
    }
    const bool use_plane = plane_ok(s, d) && !(flags & KGDET_DCN_EXACT_FP32);
    const bool use_gather = !use_plane && !(flags & KGDET_DCN_EXACT_FP32) && gather_ok(s, d) && fwd_slots_ok(s, d);
    for (int g = 0; g < s->groups; ++g) {
      DcnProblem p = forward_problem(s, d, g, inputs[i], offsets[i], masks ? masks[i] : nullptr, packed_weights[i],
                                     biases ? biases[i] : nullptr, outputs[i], flags, use_plane || use_gather);
      if (use_plane) {
        // a workgroup writes one slab per range its slice meets: keep that within kSlabSlots
        if (grp.n > 0 && !slab_slots_fit(grp.unit_begin[grp.n] + p.total_units, G, std::min(p.chunks_per_tile, group_min_len(grp))))
          if (int rc = flush()) return rc;
        // tap records: shared with an earlier problem of the group that samples at the same positions
        p.taps = nullptr;
        p.build_taps = 0;
        for (int q = 0; q < grp.n && !p.taps; ++q)
          if (grp.p[q].offset == p.offset && grp.p[q].mask == p.mask && same_geometry(grp_shape[q], s, true)) p.taps = grp.p[q].taps;
        if (!p.taps) {
          const size_t tb = tap_table_bytes(s, d);
          if (table_used + tb > table_cap) {
            set_error("workspace too small for the tap records: need %zu bytes, got %zu (kgdet_dcn_group_workspace_bytes)",
                      slab_bytes() + table_used + tb, workspace_bytes);
            return KGDET_E_WORKSPACE;
          }
          p.taps = reinterpret_cast<const DcnTapRec *>(table_base + table_used);
          p.build_taps = 1;
          table_used += tb;
        }
        grp_shape[grp.n] = s;
        append_problem(grp, p);
        lds = std::max(lds, dcn_fwd_plane_lds_bytes(parts, s->H * s->W));
        if (grp.n == kMaxFwdGroup)
          if (int rc = flush()) return rc;
      } else if (use_gather) {
        // map beyond the LDS plane: split operands, producers gather from a pixel-major copy of x (one launch per problem)
        if (int rc = flush()) return rc;
        const size_t tb = gather_table_bytes(s, d), ib = gather_image_bytes(s);
        if (tb + ib > table_cap) {
          set_error("workspace too small for the large-map forward: need %zu bytes, got %zu (kgdet_dcn_workspace_bytes)",
                    slab_bytes() + tb + ib, workspace_bytes);
          return KGDET_E_WORKSPACE;
        }
        float *xT = reinterpret_cast<float *>(table_base + tb);
        const long long HW = (long long)s->H * s->W;
        if (g == 0)
          hipLaunchKernelGGL(dcn_to_pixel_major, dim3((unsigned)((HW + 31) / 32), (s->C + 31) / 32, s->N), dim3(256), 0,
                             (hipStream_t)stream, inputs[i], xT, s->C, HW, (long long)s->C * HW);
        p.x = xT;
        p.taps = reinterpret_cast<const DcnTapRec *>(table_base);
        p.build_taps = g == 0;
        DcnFwdGroup gg = empty_group(kSlabSlots, 1, dcn_plane_wave_layout());
        append_problem(gg, p);
        if (!slab_slots_fit(p.total_units, G, p.chunks_per_tile)) {
          set_error("large-map forward: more tiles per workgroup than slab slots");
          return KGDET_E_UNSUPPORTED;
        }
        plan_static_ranges(gg, G, false, kSlabSlots - 2);
        if (int rc = allow_lds<dcn_fwd_gather<1>, dcn_fwd_gather<2>>(kMaxLds)) return rc;
        if (p.build_taps) hipLaunchKernelGGL(dcn_build_taps, dim3(2 * G, 1), dim3(256), 0, (hipStream_t)stream, gg);
        const size_t glds = dcn_fwd_plane_fixed_lds_bytes(parts);
        if (parts == 1)
          hipLaunchKernelGGL(dcn_fwd_gather<1>, dim3(G), dim3(dcn_fwd_plane_threads()), glds, (hipStream_t)stream, gg,
                             (float *)workspace);
        else
          hipLaunchKernelGGL(dcn_fwd_gather<2>, dim3(G), dim3(dcn_fwd_plane_threads()), glds, (hipStream_t)stream, gg,
                             (float *)workspace);
        launch_plane_fixup(gg, workspace, G, stream);
      } else {  // exact-fp32 kernel: one launch per problem (slabs are shared, so flush the pending group first)
        if (int rc = flush()) return rc;
        DcnFwdGroup one = empty_group(2, 0, 0, 0);
        append_problem(one, p);
        hipLaunchKernelGGL(dcn_fwd_mfma, dim3(G), dim3(kThreads), 0, (hipStream_t)stream, p, (float *)workspace);
        hipLaunchKernelGGL(dcn_fwd_fixup, dim3(one.tile_begin[1], 16), dim3(kThreads), 0, (hipStream_t)stream, one,
                           (const float *)workspace, G);
      }
    }
  }
  if (int rc = flush()) return rc;
  KGDET_CHECK_LAUNCH("dcn_fwd");
  return KGDET_OK;
}

int kgdet_deform_conv_forward(const kgdet_dcn_shape *s, const float *input, const float *offset,
                              const float *mask, const float *packed_weight, const float *bias,
                              float *output, uint32_t flags, void *workspace, size_t workspace_bytes,
                              void *stream) {
  KGDET_CHECK_SHAPE(s != nullptr, "null shape");
  return kgdet_deform_conv_forward_grouped(1, &s, &input, &offset, &mask, &packed_weight, &bias, &output, flags,
                                           workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// grad_input and grad_offset on the plane kernels
// ---------------------------------------------------------------------------------------------------------------------
int kgdet_deform_conv_grad_input(const kgdet_dcn_shape *s, const float *offset, const float *mask,
                                 const float *packed_weight, const float *grad_output, float *grad_input,
                                 uint32_t flags, void *workspace, size_t workspace_bytes, void *stream) {
  Derived d;
  if (int rc = derive(s, d)) return rc;
  KGDET_CHECK_SHAPE(offset && packed_weight && grad_output && grad_input, "null pointer");
  if (!plane_bwd_input_ok(s, d)) {
    set_error("grad_input plane kernel: maps of at most %d pixels, at most %d (weight group, deformable group) channel runs, "
              "each starting on a 256-channel tile or ending inside one", kPlaneMaxHW, kMaxFwdGroup);
    return KGDET_E_UNSUPPORTED;
  }
  const InvTables it = inv_tables(s, d);
  if (workspace == nullptr || workspace_bytes < slab_bytes() + bwd_input_table_bytes(s, d)) {
    set_error("workspace too small: need %zu bytes, got %zu", slab_bytes() + bwd_input_table_bytes(s, d), workspace_bytes);
    return KGDET_E_WORKSPACE;
  }
  unsigned char *base = (unsigned char *)workspace + slab_bytes();     // [DG] inverse tables
  unsigned char *sums_base = base + inv_tables_all(s, d);              // [DG] Gov tables, then the pixel-major grad_output
  float *gout_t = (float *)(sums_base + (size_t)s->deformable_groups * inv_gov_bytes(s, d));
  auto tables_of = [&](int dgi) { return InvTablePtrs(base + (size_t)dgi * it.stride(), it); };
  auto gov_of = [&](int dgi) { return (float *)(sums_base + (size_t)dgi * inv_gov_bytes(s, d)); };
  if (int rc = allow_lds<dcn_build_inverse_taps>(kMaxLds - 64)) return rc;
  if (int rc = allow_lds<dcn_bwd_input_plane<1>, dcn_bwd_input_plane<2>>(kMaxLds)) return rc;
  for (int dgi = 0; dgi < s->deformable_groups; ++dgi) {  // inverse sampling records from the forward geometry, per deformable group
    DcnProblem f;
    fill_problem(s, d, 0, f);
    f.offset = offset; f.mask = mask; f.dgi = dgi;
    const InvTablePtrs t = tables_of(dgi);
    hipLaunchKernelGGL(dcn_build_inverse_taps, dim3(s->N * d.K), dim3(256),
                       dcn_build_inverse_taps_lds_bytes(s->H * s->W, d.Ho * d.Wo), (hipStream_t)stream, f, t.rec, t.hdr, t.cells,
                       t.spill);
  }
  {   // sums of the cells with more than 8 contributions, for all output channels (dcn_backward_plane.hip)
    DcnPixelMajorGroup pm;
    pm.n = 1;
    pm.e[0] = gout_pixel_major(s, d, grad_output, gout_t);
    hipLaunchKernelGGL(dcn_gout_pixel_major_multi, dim3(ceil_div(d.Ho * d.Wo, 32), ceil_div(s->O, 32), s->N), dim3(256), 0,
                       (hipStream_t)stream, pm);
    DcnInvSumGroup sg;
    sg.n = 0;
    sg.sched.on = 0; sg.hot_gemm = 0;
    auto launch_sums = [&]() {
      hipLaunchKernelGGL(dcn_inv_medium_sums, dim3(s->N * d.K, kInvSumSplit, sg.n), dim3(256), 0, (hipStream_t)stream, sg);
      hipLaunchKernelGGL(dcn_inv_overflow_sums, dim3(s->N * d.K, kInvSumSplit, sg.n), dim3(256), 0, (hipStream_t)stream, sg);
      sg.n = 0;
    };
    for (int dgi = 0; dgi < s->deformable_groups; ++dgi) {
      if (sg.n == kMaxFwdGroup) launch_sums();
      const InvTablePtrs t = tables_of(dgi);
      sg.e[sg.n++] = DcnInvSum{t.hdr, t.cells, t.spill, gout_t, gov_of(dgi), s->N * d.K, d.K, d.Ho * d.Wo, s->O,
                               d.Og, d.Og_pad16, inv_gov_ld(s, d), inv_gov_slots(s, d), s->W};
    }
    launch_sums();
  }
  const int G = grid_size();
  const int parts = (flags & KGDET_DCN_BF16) ? 1 : 2;
  // (wave layout: plane_role's accumulator layout; slabs are decoded by dcn_fwd_fixup)
  DcnFwdGroup grp = empty_group(kSlabSlots, 0, dcn_plane_wave_layout());
  ChannelRun runs[kMaxFwdGroup];
  const int n_runs = channel_runs(s, d, runs, kMaxFwdGroup);
  for (int r = 0; r < n_runs; ++r)
    append_problem(grp, grad_input_problem(s, d, runs[r], grad_output, grad_input, packed_weight, tables_of(runs[r].dgi).rec,
                                           gov_of(runs[r].dgi)));
  const size_t lds = plan_plane_lds(grp, dcn_bwd_input_plane_lds_bytes(parts, d.Ho * d.Wo),
                                    dcn_bwd_input_plane_fixed_lds_bytes(parts));
  const int threads = dcn_fwd_plane_threads();
  const int Gs = small_launch_grid(grp, G);
  plan_static_ranges(grp, Gs, false, kSlabSlots - 2);
  if (parts == 1)
    hipLaunchKernelGGL(dcn_bwd_input_plane<1>, dim3(Gs), dim3(threads), lds, (hipStream_t)stream, grp, (float *)workspace);
  else
    hipLaunchKernelGGL(dcn_bwd_input_plane<2>, dim3(Gs), dim3(threads), lds, (hipStream_t)stream, grp, (float *)workspace);
  launch_plane_fixup(grp, workspace, Gs, stream);
  KGDET_CHECK_LAUNCH("dcn_bwd_input_plane");
  return KGDET_OK;
}

// v1 (mask == nullptr) or v2 (mask, grad_mask; split operands and static ranges only: KGDET_E_UNSUPPORTED otherwise, before
// anything is launched)
static int grad_offset_plane(const kgdet_dcn_shape *s, const float *input, const float *offset, const float *mask,
                             const float *packed_weight, const float *grad_output, float *grad_offset, float *grad_mask,
                             uint32_t flags, void *workspace, size_t workspace_bytes, void *stream) {
  Derived d;
  if (int rc = derive(s, d)) return rc;
  KGDET_CHECK_SHAPE(input && offset && packed_weight && grad_output && grad_offset, "null pointer");
  KGDET_CHECK_SHAPE((mask == nullptr) == (grad_mask == nullptr), "mask and grad_mask must come together");
  if (!plane_bwd_offset_ok(s, d, mask != nullptr) || (mask && (flags & KGDET_DCN_BF16))) {
    set_error("grad_offset plane kernel: needs every deformable group inside one weight group (whole 16-channel chunks), "
              "<= 256 output channels per group, H*W <= %d", kPlaneMaxHW);
    return KGDET_E_UNSUPPORTED;
  }
  const size_t need = slab_bytes() + grad_tap_bytes(s, d);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    return KGDET_E_WORKSPACE;
  }
  if (int rc = allow_lds<dcn_bwd_offset_plane<1>, dcn_bwd_offset_plane<2>, dcn_bwd_offset_plane_masked>(kMaxLds)) return rc;
  const int G = grid_size();
  const int parts = (flags & KGDET_DCN_BF16) ? 1 : 2;
  DcnFwdGroup grp = empty_group(kSlabSlots, 0, 0);
  // one sub-problem per deformable group (= channel run: plane_bwd_offset_ok), each with its own record table
  unsigned char *const recs = (unsigned char *)workspace + slab_bytes();
  ChannelRun runs[kMaxFwdGroup];
  const int n_runs = channel_runs(s, d, runs, kMaxFwdGroup);
  for (int r = 0; r < n_runs; ++r)
    append_problem(grp, grad_offset_problem(s, d, runs[r], input, offset, mask, packed_weight, grad_output, grad_offset, grad_mask,
                                            recs + (size_t)runs[r].dgi * grad_tap_stride(s, d), true, flags));
  const int Gs = mask ? G : small_launch_grid(grp, G);      // (v2 needs one workgroup per range: the full grid)
  plan_static_ranges(grp, Gs, mask != nullptr);
  if (mask && !grp.static_ranges) {
    set_error("grad_offset plane kernel (v2): more (part, tile) ranges than workgroups");
    return KGDET_E_UNSUPPORTED;
  }
  const bool use_pair = parts == 2 && !mask && offset_pair_ok(grp);
  if (use_pair) place_offset_xblk(grp, recs, grad_tap_bytes(s, d), workspace_bytes - slab_bytes());
  note_offset_handover(grp, use_pair);
  hipLaunchKernelGGL(dcn_build_grad_taps, dim3(2 * G, grp.n), dim3(256), 0, (hipStream_t)stream, grp);
  const size_t lds = dcn_bwd_offset_plane_lds_bytes(parts, d.K, s->H * s->W, mask != nullptr);
  const int threads = dcn_bwd_offset_plane_threads();
  if (mask) {
    hipLaunchKernelGGL(dcn_bwd_offset_plane_masked, dim3(G), dim3(threads), lds, (hipStream_t)stream, grp, (float *)workspace,
                       d.K);
    hipLaunchKernelGGL(dcn_bwd_offset_plane_fixup_masked, dim3(grp.tile_begin[grp.n], 8), dim3(256), 0, (hipStream_t)stream,
                       grp, (const float *)workspace, G, d.K);
    KGDET_CHECK_LAUNCH("dcn_bwd_offset_plane_masked");
    return KGDET_OK;
  }
  if (parts == 1)
    hipLaunchKernelGGL(dcn_bwd_offset_plane<1>, dim3(Gs), dim3(threads), lds, (hipStream_t)stream, grp,
                       (float *)workspace, d.K);
  else if (use_pair) {
    if (int rc = launch_offset_pair(grp, Gs, workspace, d.K, stream)) return rc;
  } else
    hipLaunchKernelGGL(dcn_bwd_offset_plane<2>, dim3(Gs), dim3(threads), lds, (hipStream_t)stream, grp,
                       (float *)workspace, d.K);
  hipLaunchKernelGGL(dcn_bwd_offset_plane_fixup, dim3(grp.tile_begin[grp.n], 8), dim3(256), 0, (hipStream_t)stream, grp,
                     (const float *)workspace, Gs, d.K);
  KGDET_CHECK_LAUNCH("dcn_bwd_offset_plane");
  return KGDET_OK;
}

int kgdet_deform_conv_grad_offset(const kgdet_dcn_shape *s, const float *input, const float *offset,
                                  const float *packed_weight, const float *grad_output, float *grad_offset,
                                  uint32_t flags, void *workspace, size_t workspace_bytes, void *stream) {
  return grad_offset_plane(s, input, offset, nullptr, packed_weight, grad_output, grad_offset, nullptr, flags, workspace,
                           workspace_bytes, stream);
}

// test hook: with KGDET_DCN_HOT_DEBUG=1 in the environment, the grouped backward copies (synchronously, before its second phase
// reuses the tables) how many hot cells its builder handed to dcn_hot_gemm, per (distinct offset tensor, image) in launch order; this
// returns the last call's counts (raw: values above kHotMaxCols mean the rest went the cluster path).
namespace { struct HotDbg { const int *ptr[kMaxFwdGroup]; int N[kMaxFwdGroup]; int n; int vals[64]; int n_vals; }; HotDbg g_hot_dbg = {}; }
int kgdet_debug_dcn_hot_columns(int *out, int max_out) {
  int w = 0;
  for (; w < g_hot_dbg.n_vals && w < max_out; ++w) out[w] = g_hot_dbg.vals[w];
  return w;
}

int kgdet_debug_dcn_offset_handover(void) { return g_offset_handover; }

// n v1 problems: grad_input of all of them in one dcn_bwd_input_plane launch, grad_offset of all of them in one
// dcn_bwd_offset_plane launch (inverse / gradient records are built once per distinct offset tensor).
int kgdet_deform_conv_backward_input_grouped(int32_t n, const kgdet_dcn_shape *const *shapes, const float *const *inputs,
                                             const float *const *offsets, const float *const *packed_weights,
                                             const float *const *grad_outputs, float *const *grad_inputs,
                                             float *const *grad_offsets, void *workspace, size_t workspace_bytes,
                                             void *stream) {
  KGDET_CHECK_SHAPE(n >= 1 && n <= kMaxFwdGroup && shapes && inputs && offsets && packed_weights && grad_outputs &&
                        grad_inputs && grad_offsets, "null pointer / group size not in [1, %d]", kMaxFwdGroup);
  const int G = grid_size();
  Derived dd[kMaxFwdGroup];
  int same_as[kMaxFwdGroup];  // earlier problem with the same offsets and geometry (shares its records)
  size_t inv_off[kMaxFwdGroup], rec_off[kMaxFwdGroup], sum_off[kMaxFwdGroup], inv_total = 0, rec_total = 0;
  int max_K = 0;
  for (int i = 0; i < n; ++i) {
    const kgdet_dcn_shape *s = shapes[i];
    if (int rc = derive(s, dd[i])) return rc;
    KGDET_CHECK_SHAPE(inputs[i] && offsets[i] && packed_weights[i] && grad_outputs[i] && grad_inputs[i] &&
                          grad_offsets[i], "null pointer (problem %d)", i);
    if (s->groups != 1 || s->deformable_groups != 1 || !plane_bwd_input_ok(s, dd[i]) || !plane_bwd_offset_ok(s, dd[i])) {
      set_error("problem %d is not eligible for the plane backward kernels", i);
      return KGDET_E_UNSUPPORTED;
    }
    same_as[i] = -1;
    for (int q = 0; q < i && same_as[i] < 0; ++q)
      if (offsets[q] == offsets[i] && same_geometry(shapes[q], s, false)) same_as[i] = same_as[q] >= 0 ? same_as[q] : q;
    if (same_as[i] < 0) {
      inv_off[i] = inv_total; inv_total += inv_tables(s, dd[i]).stride();
      rec_off[i] = rec_total; rec_total += align_up(grad_tap_bytes(s, dd[i]), 256);
    } else {
      inv_off[i] = inv_off[same_as[i]]; rec_off[i] = rec_off[same_as[i]];
    }
    max_K = std::max(max_K, dd[i].K);
  }
  for (int i = 0; i < n; ++i) {   // per problem (functions of its grad_output): the long cells' sums + the pixel-major grad_output
    sum_off[i] = inv_total; inv_total += inv_sums_all(shapes[i], dd[i]);
  }
  const size_t tables = std::max(inv_total, rec_total);  // the two phases run one after the other
  if (workspace == nullptr || workspace_bytes < slab_bytes() + tables) {
    set_error("workspace too small: need %zu bytes, got %zu (kgdet_dcn_group_workspace_bytes)", slab_bytes() + tables,
              workspace_bytes);
    return KGDET_E_WORKSPACE;
  }
  if (int rc = allow_lds<dcn_build_inverse_taps>(kMaxLds - 64)) return rc;
  if (int rc = allow_lds<dcn_bwd_input_plane<2>, dcn_bwd_offset_plane<2>>(kMaxLds)) return rc;
  unsigned char *tab = (unsigned char *)workspace + slab_bytes();

  // ---- phase 1: grad_input (transposed sampling) ----
  // (wave layout: plane_role's accumulator layout; slabs are decoded by dcn_fwd_fixup)
  DcnFwdGroup grp = empty_group(kSlabSlots, 0, dcn_plane_wave_layout());
  size_t lds = 0;
  DcnInvBuildGroup builds;
  builds.n = 0;
  int build_blocks = 0;
  size_t build_lds = 0;
  DcnPixelMajorGroup pmg;      // grad_output windows -> pixel-major copies, one launch
  pmg.n = 0;
  int pm_px = 0, pm_c = 0, pm_images = 0;
  DcnInvSumGroup sums;         // the long cells' sums of every problem, one launch
  sums.n = 0;
  // (problem, image) groups onto XCDs, largest first onto the least loaded one (DcnInvSumSched): the sums kernel and the hot-cell GEMM
  // both read a group's 1 MB pixel-major grad_output from one XCD's L2
  int sched_longest = 0;
  {
    static const bool xcd_off = env_int("KGDET_DCN_SUMS_XCD", 1) == 0;   // A/B switch
    DcnInvSumSched &sc = sums.sched;
    sc.on = 0;
    int load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int x = 0; x < 8; ++x) sc.n_seg[x] = 0;
    // (KGDET_DCN_SUMS_HALVES=1, measured and left off: every pair as TWO segments -- its first and second half of the taps; six
    // problems x two images are 12 pairs for 8 XCDs.  dcn_inv_medium_sums 43.6 against 44.1 us, dcn_hot_gemm 36 against 21 us)
    struct G_ { int z, b, units, u0; } gs[kMaxFwdGroup * 128];
    int ng = 0;
    bool fits = !xcd_off;
    for (int z = 0; z < n && fits; ++z)
      for (int b = 0; b < shapes[z]->N && fits; ++b) {
        if (ng + 2 > kMaxFwdGroup * 128) { fits = false; break; }
        static const bool no_halves = env_int("KGDET_DCN_SUMS_HALVES", 0) != 1;   // (experiment, off)
        const int units = dd[z].K * kInvSumSplit, h0 = no_halves ? units : (dd[z].K + 1) / 2 * kInvSumSplit;
        gs[ng++] = G_{z, b, h0, 0};
        if (units > h0) gs[ng++] = G_{z, b, units - h0, h0};
      }
    std::stable_sort(gs, gs + ng, [](const G_ &a, const G_ &b) { return a.units > b.units; });
    for (int i = 0; i < ng && fits; ++i) {
      int x = 0;
      for (int y = 1; y < 8; ++y) if (load[y] < load[x]) x = y;
      if (sc.n_seg[x] >= kInvSumSegs) { fits = false; break; }
      sc.seg[x][sc.n_seg[x]++] = DcnInvSumSeg{gs[i].z, gs[i].b, load[x], gs[i].units, gs[i].u0};
      load[x] += gs[i].units;
    }
    if (fits) {
      sc.on = 1;
      for (int x = 0; x < 8; ++x) sched_longest = std::max(sched_longest, load[x]);
    }
  }
  static const bool hot_off = env_int("KGDET_DCN_HOT_GEMM", 1) == 0;   // A/B switch
  bool hot_ok = !hot_off;       // hot cells (> 64 contributions) as one GEMM per (problem, image): dcn_hot_gemm
  g_hot_dbg.n = 0; g_hot_dbg.n_vals = 0;
  // (test switch, read on every call: a shorter column list, to reach the overflow rule with small kernels)
  const int hot_max = std::max(32, std::min(kHotMaxCols, env_int("KGDET_DCN_HOT_MAX_COLS", kHotMaxCols)));
  hot_ok = hot_ok && sums.sched.on;   // (its workgroups follow the same XCD schedule)
  for (int i = 0; i < n; ++i) hot_ok = hot_ok && inv_gov_ld(shapes[i], dd[i]) == shapes[i]->O;
  DcnHotGemmGroup hotg;
  hotg.n = 0;
  int sums_blocks = 0;
  for (int i = 0; i < n; ++i) {
    const kgdet_dcn_shape *s = shapes[i];
    const Derived &d = dd[i];
    const InvTablePtrs t(tab + inv_off[i], inv_tables(s, d));
    float *gov = (float *)(tab + sum_off[i]);
    float *gout_t = (float *)(tab + sum_off[i] + inv_gov_bytes(s, d));
    pmg.e[pmg.n++] = gout_pixel_major(s, d, grad_outputs[i], gout_t);
    pm_px = std::max(pm_px, d.Ho * d.Wo); pm_c = std::max(pm_c, s->O); pm_images += s->N;
    // (the column list lives with the offset tensor's records: t.hot_cols / t.hot_count also for a problem that shares them)
    sums.e[sums.n++] = DcnInvSum{t.hdr, t.cells, t.spill, gout_t, gov, s->N * d.K, d.K, d.Ho * d.Wo, s->O, d.Og, d.Og_pad16,
                                 inv_gov_ld(s, d), inv_gov_slots(s, d), s->W, hot_ok ? t.hot_count : nullptr, hot_ok ? hot_max : 0};
    sums_blocks = std::max(sums_blocks, s->N * d.K);
    hotg.e[hotg.n++] = DcnHotGemm{t.hot_cols, t.hot_count, t.spill, gout_t, gov, s->N, d.K, d.Ho * d.Wo, s->O, inv_gov_ld(s, d),
                                  inv_gov_slots(s, d), hot_max};
    if (same_as[i] < 0) {   // (all distinct offset tensors of the group: one builder launch below)
      DcnInvBuild &e = builds.e[builds.n++];
      fill_problem(s, d, 0, e.p);
      e.p.offset = offsets[i]; e.p.mask = nullptr;
      e.inv = t.rec; e.hdr = t.hdr; e.cells = t.cells; e.spill = t.spill;
      e.hot_cols = hot_ok ? t.hot_cols : nullptr;
      e.hot_count = hot_ok ? t.hot_count : nullptr;
      e.hot_max = hot_max;
      if (hot_ok) {
        KGDET_HIP_TRY(hipMemsetAsync(e.hot_count, 0, (size_t)s->N * sizeof(int), (hipStream_t)stream));
        if (g_hot_dbg.n < kMaxFwdGroup) { g_hot_dbg.ptr[g_hot_dbg.n] = e.hot_count; g_hot_dbg.N[g_hot_dbg.n++] = s->N; }
      }
      build_blocks = std::max(build_blocks, s->N * d.K);
      build_lds = std::max(build_lds, dcn_build_inverse_taps_lds_bytes(s->H * s->W, d.Ho * d.Wo));
    }
    append_problem(grp, grad_input_problem(s, d, ChannelRun{0, s->C, 0, 0}, grad_outputs[i], grad_inputs[i], packed_weights[i],
                                           t.rec, gov));
    lds = std::max(lds, dcn_bwd_input_plane_lds_bytes(2, d.Ho * d.Wo));
  }
  if (!slab_slots_fit(grp.unit_begin[grp.n], G, group_min_len(grp))) { set_error("group too uneven for the slab slots"); return KGDET_E_UNSUPPORTED; }
  // problems that share a grad_input pointer are summed into it by the fix-up (sum groups); planned before anything is launched
  if (!assign_sum_groups(grp, (const void *const *)grad_inputs, false)) {
    set_error("aliased grad_input pointers: the problems do not tile alike (or more than four share one)");
    return KGDET_E_UNSUPPORTED;
  }
  lds = plan_plane_lds(grp, lds, dcn_bwd_input_plane_fixed_lds_bytes(2));
  const int Gs = small_launch_grid(grp, G);
  plan_static_ranges(grp, Gs, false, kSlabSlots - 2);
  if (has_sum_groups(grp) && !grp.static_ranges) {
    set_error("aliased grad_input pointers need the static schedule (one range per workgroup)");
    return KGDET_E_UNSUPPORTED;
  }
  const int only_phase = g_options[KGDET_OPT_BWD_PHASE];   // (measurement switch: 1 = grad_input only, 2 = grad_offset only)
  if (only_phase != 2) {
    {
      static const bool fused_off = env_int("KGDET_DCN_BWD_PREPARE", 1) == 0;   // A/B switch
      if (int rc = allow_lds<dcn_build_inverse_taps_multi>(kMaxLds - 64)) return rc;
      if (int rc = allow_lds<dcn_bwd_input_prepare>(kMaxLds - 64 - 2 * 32 * 33 * 4 - 64)) return rc;
      const int pm_bx = ceil_div(pm_px, 32), pm_by = ceil_div(pm_c, 32);
      if (!fused_off && build_lds + 2 * 32 * 33 * 4 + 128 <= kMaxLds - 64) {
        const int pm_blocks = ceil_div(pm_bx * pm_by * pm_images, 2);
        hipLaunchKernelGGL(dcn_bwd_input_prepare, dim3(build_blocks * builds.n + pm_blocks), dim3(512), build_lds, (hipStream_t)stream,
                           builds, pmg, build_blocks, pm_bx, pm_by);
      } else {
        if (builds.n > 0)
          hipLaunchKernelGGL(dcn_build_inverse_taps_multi, dim3(build_blocks, builds.n), dim3(256), build_lds, (hipStream_t)stream,
                             builds);
        hipLaunchKernelGGL(dcn_gout_pixel_major_multi, dim3(pm_bx, pm_by, pm_images), dim3(256), 0, (hipStream_t)stream, pmg);
      }
    }
    sums.hot_gemm = hot_ok ? 1 : 0;
    if (hot_ok) {
      if (int rc = allow_lds<dcn_hot_gemm>(dcn_hot_gemm_lds_bytes())) return rc;
      hipLaunchKernelGGL(dcn_hot_gemm, dim3(8 * kHotBlocksPerXcd), dim3(512), dcn_hot_gemm_lds_bytes(), (hipStream_t)stream, hotg,
                         sums.sched);
    }
    // the cluster kernel serves the cells above 64 contributions that dcn_hot_gemm does not take: none, if the GEMM is on and no image
    // can overflow its column list (a tap has at most 4 HoWo / 65 such cells)
    bool clusters_needed = !hot_ok;
    for (int i = 0; i < n && !clusters_needed; ++i)
      clusters_needed = (long long)dd[i].K * (4 * dd[i].Ho * dd[i].Wo / 65) > hot_max;
    if (sums.sched.on) {
      hipLaunchKernelGGL(dcn_inv_medium_sums, dim3(8 * sched_longest), dim3(256), 0, (hipStream_t)stream, sums);
      if (clusters_needed)
        hipLaunchKernelGGL(dcn_inv_overflow_sums, dim3(8 * sched_longest), dim3(256), 0, (hipStream_t)stream, sums);
    } else {
      hipLaunchKernelGGL(dcn_inv_medium_sums, dim3(sums_blocks, kInvSumSplit, sums.n), dim3(256), 0, (hipStream_t)stream, sums);
      hipLaunchKernelGGL(dcn_inv_overflow_sums, dim3(sums_blocks, kInvSumSplit, sums.n), dim3(256), 0, (hipStream_t)stream, sums);
    }
    if (g_hot_dbg.n > 0 && env_int("KGDET_DCN_HOT_DEBUG", 0) == 1) {   // (test hook, see above; read on every call)
      KGDET_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
      for (int i = 0; i < g_hot_dbg.n; ++i)
        for (int b = 0; b < g_hot_dbg.N[i] && g_hot_dbg.n_vals < 64; ++b)
          KGDET_HIP_TRY(hipMemcpy(&g_hot_dbg.vals[g_hot_dbg.n_vals++], g_hot_dbg.ptr[i] + b, sizeof(int), hipMemcpyDeviceToHost));
    }
    hipLaunchKernelGGL(dcn_bwd_input_plane<2>, dim3(Gs), dim3(dcn_fwd_plane_threads()), lds, (hipStream_t)stream, grp,
                       (float *)workspace);
    launch_plane_fixup(grp, workspace, Gs, stream);
  }
  if (only_phase == 1) {   // (measurement switch: grad_offset was NOT written -- never reported as success)
    KGDET_CHECK_LAUNCH("dcn_bwd_plane_grouped");
    set_error("KGDET_OPT_BWD_PHASE = 1: grad_offset not computed");
    return KGDET_E_PARTIAL;
  }

  // ---- phase 2: grad_offset (column gradient in registers) ----
  grp.n = 0;
  grp.wave_layout = 0;
  grp.static_ranges = 0;
  lds = 0;
  for (int i = 0; i < n; ++i) {
    const kgdet_dcn_shape *s = shapes[i];
    append_problem(grp, grad_offset_problem(s, dd[i], ChannelRun{0, s->C, 0, 0}, inputs[i], offsets[i], nullptr, packed_weights[i],
                                            grad_outputs[i], grad_offsets[i], nullptr, tab + rec_off[i], same_as[i] < 0, 0));
    lds = std::max(lds, dcn_bwd_offset_plane_lds_bytes(2, max_K, s->H * s->W));
  }
  if (lds > kMaxLds || !slab_slots_fit(grp.unit_begin[grp.n], G, group_min_len(grp))) {
    set_error("group does not fit the grad_offset kernel");
    return KGDET_E_UNSUPPORTED;
  }
  if (!assign_sum_groups(grp, (const void *const *)grad_offsets, true)) {
    set_error("aliased grad_offset pointers: the problems do not tile alike (or more than four share one)");
    return KGDET_E_UNSUPPORTED;
  }
  const int Go = small_launch_grid(grp, G);
  plan_static_ranges(grp, Go);
  if (has_sum_groups(grp) && !grp.static_ranges) {
    set_error("aliased grad_offset pointers need the static schedule (one range per workgroup)");
    return KGDET_E_UNSUPPORTED;
  }
  const bool use_pair = offset_pair_ok(grp);
  if (use_pair) place_offset_xblk(grp, tab, rec_total, workspace_bytes - slab_bytes());
  note_offset_handover(grp, use_pair);
  hipLaunchKernelGGL(dcn_build_grad_taps, dim3(2 * G, grp.n), dim3(256), 0, (hipStream_t)stream, grp);
  if (use_pair) {
    if (int rc = launch_offset_pair(grp, Go, workspace, max_K, stream)) return rc;
  } else
    hipLaunchKernelGGL(dcn_bwd_offset_plane<2>, dim3(Go), dim3(dcn_bwd_offset_plane_threads()), lds, (hipStream_t)stream, grp,
                       (float *)workspace, max_K);
  hipLaunchKernelGGL(dcn_bwd_offset_plane_fixup, dim3(grp.tile_begin[grp.n], 8), dim3(256), 0, (hipStream_t)stream, grp,
                     (const float *)workspace, Go, max_K);
  KGDET_CHECK_LAUNCH("dcn_bwd_plane_grouped");
  if (only_phase == 2) {   // (measurement switch: grad_input was NOT written)
    set_error("KGDET_OPT_BWD_PHASE = 2: grad_input not computed");
    return KGDET_E_PARTIAL;
  }
  return KGDET_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// grad_weight on the split-operand kernels
// ---------------------------------------------------------------------------------------------------------------------
// grad_weight of n problems in one launch of the plane kernel (+ record / grad_out image builders, fix-up).
// masks: nullptr (v1) or one mask pointer per problem (v2: the tap records carry mask x bilinear weight)
// Weight groups and deformable groups: a problem is cut into runs of input channels that share both (sub-problems: the
// input window, the weight group's grad_out image and output rows, the deformable group's tap records); at most
// kMaxFwdGroup sub-problems per launch.
// gather: one problem on a map beyond the LDS plane -- pixel-major copy of x behind the tables, dcn_bwd_weight_gather.
static int grad_weight_plane_grouped(int32_t n, const kgdet_dcn_shape *const *shapes, const float *const *inputs,
                                     const float *const *offsets, const float *const *masks, const float *const *grad_outputs,
                                     float *const *grad_weights, void *workspace, size_t workspace_bytes, void *stream,
                                     bool gather = false) {
  KGDET_CHECK_SHAPE(n >= 1 && n <= kMaxFwdGroup && shapes && inputs && offsets && grad_outputs && grad_weights,
                    "null pointer / group size not in [1, %d]", kMaxFwdGroup);
  KGDET_CHECK_SHAPE(!gather || n == 1, "the large-map grad_weight kernel takes one problem per launch");
  const int G = grid_size();
  Derived dd[kMaxFwdGroup];
  ChannelRun runs[kMaxFwdGroup][kMaxFwdGroup];   // per problem (the first kMaxFwdGroup: more are refused below)
  int n_runs[kMaxFwdGroup];
  int same_taps[kMaxFwdGroup], same_gq[kMaxFwdGroup];
  size_t taps_off[kMaxFwdGroup], gq_off[kMaxFwdGroup], total = 0;
  int n_sub = 0;
  for (int i = 0; i < n; ++i) {
    const kgdet_dcn_shape *s = shapes[i];
    if (int rc = derive(s, dd[i])) return rc;
    KGDET_CHECK_SHAPE(inputs[i] && offsets[i] && grad_outputs[i] && grad_weights[i], "null pointer (problem %d)", i);
    if (!(gather ? gather_ok(s, dd[i]) : plane_ok(s, dd[i])) || dd[i].K > 128) {   // (the fix-up: at most 16 tap groups per channel chunk)
      set_error("problem %d is not eligible for the plane grad_weight kernel", i);
      return KGDET_E_UNSUPPORTED;
    }
    n_runs[i] = channel_runs(s, dd[i], runs[i], kMaxFwdGroup);
    n_sub += n_runs[i];
    same_taps[i] = same_gq[i] = -1;
    for (int q = 0; q < i; ++q) {
      const kgdet_dcn_shape *o = shapes[q];
      if (same_taps[i] < 0 && same_geometry(o, s, true) && offsets[q] == offsets[i] && (!masks || masks[q] == masks[i]))
        same_taps[i] = same_taps[q] >= 0 ? same_taps[q] : q;
      if (same_gq[i] < 0 && grad_outputs[q] == grad_outputs[i] && o->N == s->N && o->O == s->O && o->groups == s->groups &&
          o->out_channel_offset == s->out_channel_offset && o->out_channels_total == s->out_channels_total &&
          dd[q].Ho == dd[i].Ho && dd[q].Wo == dd[i].Wo)
        same_gq[i] = same_gq[q] >= 0 ? same_gq[q] : q;
    }
    if (same_taps[i] < 0) { taps_off[i] = total; total += gather ? gather_table_bytes(s, dd[i]) : align_up(tap_table_bytes(s, dd[i]), 256); }
    else taps_off[i] = taps_off[same_taps[i]];
    if (same_gq[i] < 0) { gq_off[i] = total; total += gq_image_bytes(s, dd[i]); }
    else gq_off[i] = gq_off[same_gq[i]];
  }
  if (n_sub > kMaxFwdGroup) {
    set_error("more than %d (weight group, deformable group) channel runs in one launch", kMaxFwdGroup);
    return KGDET_E_UNSUPPORTED;
  }
  const size_t image_off = total;   // (gather) the pixel-major copy of x
  if (gather) total += gather_image_bytes(shapes[0]);
  // Output-stationary kernel (dcn_backward_weight_os.hip, round 4): a workgroup owns a 256 x (16 channels x 13 taps) tile for
  // the whole reduction over pixels -- no partial tiles, no fix-up -- when all tiles of the call fit ONE round over the CUs
  // (a KGDet head stage: 224).  Otherwise (and KGDET_DCN_WGRAD_OS=0, A/B) the stream-K kernel + fix-up below.
  bool use_os = false;
  if (!gather) {
    static const int os_on = env_int("KGDET_DCN_WGRAD_OS", 1);
    long long os_tiles = 0;
    for (int i = 0; i < n; ++i)
      for (int r = 0; r < n_runs[i]; ++r)
        os_tiles += (long long)(dd[i].Og_pad / kTileM) * ceil_div(runs[i][r].c1 - runs[i][r].c0, kChunk) *
                    ceil_div(dd[i].K, dcn_bwd_weight_os_taps());
    use_os = os_on && g_options[KGDET_OPT_WGRAD_STREAMK] == 0 && os_tiles <= G;
  }
  if (workspace == nullptr || workspace_bytes < slab_bytes() + total) {
    set_error("workspace too small: need %zu bytes, got %zu (kgdet_dcn_group_workspace_bytes)", slab_bytes() + total,
              workspace_bytes);
    return KGDET_E_WORKSPACE;
  }
  if (int rc = allow_lds<dcn_bwd_weight_plane<2>, dcn_bwd_weight_gather<2>>(kMaxLds)) return rc;
  unsigned char *tab = (unsigned char *)workspace + slab_bytes();
  if (gather) {
    const kgdet_dcn_shape *s = shapes[0];
    const long long HW = (long long)s->H * s->W;
    hipLaunchKernelGGL(dcn_to_pixel_major, dim3((unsigned)((HW + 31) / 32), (s->C + 31) / 32, s->N), dim3(256), 0,
                       (hipStream_t)stream, inputs[0], reinterpret_cast<float *>(tab + image_off), s->C, HW, (long long)s->C * HW);
  }
  DcnFwdGroup grp = empty_group(kSlabSlots, gather ? 1 : 0, 0);
  size_t lds = 0;
  DcnPackGradOut pack;          // the grad_out images of the call: one launch (at most one per channel run: <= kMaxFwdGroup)
  int n_pack = 0, pack_x = 0, pack_y = 0;
  for (int i = 0; i < n; ++i) {
    const kgdet_dcn_shape *s = shapes[i];
    const Derived &d = dd[i];
    const int n_px16 = ceil_div(d.Ho * d.Wo, kChunk);
    int packed_group = -1;   // grad_out images of the weight groups are packed as their first channel run is met
    for (int r = 0; r < n_runs[i]; ++r) {
      const int g = runs[i][r].g;
      void *gq = tab + gq_off[i] + (size_t)g * gq_group_bytes(s, d);
      const DcnProblem p = grad_weight_problem(s, d, runs[i][r], gather ? reinterpret_cast<const float *>(tab + image_off) : inputs[i],
                                               offsets[i], masks ? masks[i] : nullptr, grad_weights[i], tab + taps_off[i],
                                               same_taps[i] < 0 && r == 0, gq, use_os ? dcn_bwd_weight_os_taps() : 8);
      if (same_gq[i] < 0 && packed_group < g) {
        DcnPackGradOutItem &it = pack.item[n_pack++];
        it.gout = grad_outputs[i]; it.gq = gq;
        it.N = s->N; it.O_total = p.O_total; it.o_base = p.o_base; it.Og = d.Og; it.HoWo = p.HoWo; it.n_px16 = n_px16;
        it.n_mtiles = d.Og_pad / kTileM;
        pack_x = std::max(pack_x, s->N * n_px16);
        pack_y = std::max(pack_y, d.Og_pad / kTileM);
        packed_group = g;
      }
      append_problem(grp, p);
    }
    const size_t need = gather ? dcn_bwd_weight_gather_lds_bytes(2)
                               : use_os ? dcn_bwd_weight_os_lds_bytes(2, s->H * s->W) : dcn_bwd_weight_plane_lds_bytes(2, s->H * s->W);
    lds = std::max(lds, need);
  }
  // The fix-up lists at most 32 slabs per tile: small problems run on fewer workgroups, so that a workgroup's share of the
  // units is at least 1/30 of the longest tile.
  int Gw = G;
  if (!use_os) {
    int max_len = 0;
    for (int i = 0; i < grp.n; ++i) max_len = std::max(max_len, grp.p[i].chunks_per_tile);
    const long long fit = grp.unit_begin[grp.n] / ceil_div(max_len, 30);
    if (fit < Gw) Gw = (int)std::max<long long>(1, fit);
    if (!slab_slots_fit(grp.unit_begin[grp.n], Gw, group_min_len(grp))) {
      set_error("group too uneven for the slab slots");
      return KGDET_E_UNSUPPORTED;
    }
  } else if (int rc = allow_lds<dcn_bwd_weight_os<2>>(kMaxLds)) {
    return rc;
  }
  if (n_pack > 0)
    hipLaunchKernelGGL(dcn_pack_grad_out, dim3(pack_x, pack_y, n_pack), dim3(256), 0, (hipStream_t)stream, pack, 2);
  hipLaunchKernelGGL(dcn_build_taps, dim3(2 * G, grp.n), dim3(256), 0, (hipStream_t)stream, grp);
  if (use_os) {
    const int Gos = ceil_div(grp.tile_begin[grp.n], 8) * 8;      // (a multiple of 8: the XCD-contiguous tile order is a bijection)
    hipLaunchKernelGGL(dcn_bwd_weight_os<2>, dim3(Gos), dim3(dcn_bwd_weight_os_threads()), lds, (hipStream_t)stream, grp);
    KGDET_CHECK_LAUNCH("dcn_bwd_weight_os");
    return KGDET_OK;
  }
  if (gather)
    hipLaunchKernelGGL(dcn_bwd_weight_gather<2>, dim3(Gw), dim3(dcn_bwd_weight_plane_threads()), lds, (hipStream_t)stream, grp,
                       (float *)workspace);
  else
    hipLaunchKernelGGL(dcn_bwd_weight_plane<2>, dim3(Gw), dim3(dcn_bwd_weight_plane_threads()), lds, (hipStream_t)stream, grp,
                       (float *)workspace);
  int fix_blocks = 0, max_K = 0;
  for (int i = 0; i < grp.n; ++i) {
    fix_blocks += (grp.p[i].n_ntiles / grp.p[i].tiles_per_image) * grp.p[i].n_mtiles * 32;
    max_K = std::max(max_K, grp.p[i].K);
  }
  const size_t fix_lds = (size_t)8 * 16 * max_K * sizeof(float);
  if (int rc = allow_lds<dcn_bwd_weight_plane_fixup>(80 * 1024)) return rc;   // (beside its static slab lists)
  hipLaunchKernelGGL(dcn_bwd_weight_plane_fixup, dim3(fix_blocks), dim3(256), fix_lds, (hipStream_t)stream, grp,
                     (const float *)workspace, Gw);
  KGDET_CHECK_LAUNCH("dcn_bwd_weight_plane");
  return KGDET_OK;
}

int kgdet_deform_conv_grad_weight_grouped(int32_t n, const kgdet_dcn_shape *const *shapes, const float *const *inputs,
                                          const float *const *offsets, const float *const *grad_outputs,
                                          float *const *grad_weights, void *workspace, size_t workspace_bytes,
                                          void *stream) {
  return grad_weight_plane_grouped(n, shapes, inputs, offsets, nullptr, grad_outputs, grad_weights, workspace, workspace_bytes,
                                   stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Dispatchers: the split-operand kernels above where they apply, the fp32 kernels otherwise
// ---------------------------------------------------------------------------------------------------------------------
int kgdet_deform_conv_backward_input(const kgdet_dcn_shape *s, const float *input, const float *offset,
                                     const float *mask, const float *packed_weight, const float *grad_output,
                                     float *grad_input, float *grad_offset, float *grad_mask, void *workspace,
                                     size_t workspace_bytes, void *stream) {
  Derived d;
  if (int rc = derive(s, d)) return rc;
  KGDET_CHECK_SHAPE(input && offset && packed_weight && grad_output && grad_input && grad_offset, "null pointer");
  KGDET_CHECK_SHAPE((mask == nullptr) == (grad_mask == nullptr), "mask and grad_mask must come together");
  // v1 on small maps: the two plane kernels (grad_input by transposed sampling, grad_offset with the column
  // gradient in registers), bf16 hi/lo split MFMA -- 2x faster than the f32 gather kernel below
  const bool plane_off = g_options[KGDET_OPT_EXACT_BACKWARD] != 0;
  if (!plane_off && plane_bwd_input_ok(s, d) && plane_bwd_offset_ok(s, d, mask != nullptr)) {
    // The route is a function of the shape and the options alone, never of the room in the workspace: a buffer too short for
    // the two plane launches is refused here, before either writes anything (a shorter buffer used to send the call down the
    // exact-fp32 kernels below: KGDET_OK with other bits for the same call).
    const size_t need = slab_bytes() + std::max(grad_tap_bytes(s, d), bwd_input_table_bytes(s, d));
    if (workspace == nullptr || workspace_bytes < need) {
      set_error("workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
      return KGDET_E_WORKSPACE;
    }
    // (grad_offset first: the v2 variant declines -- before launching anything -- when its ranges outnumber the
    // workgroups, and the gather path below then does everything)
    const int rc = grad_offset_plane(s, input, offset, mask, packed_weight, grad_output, grad_offset, grad_mask, 0, workspace,
                                     workspace_bytes, stream);
    if (rc == KGDET_OK)
      return kgdet_deform_conv_grad_input(s, offset, mask, packed_weight, grad_output, grad_input, 0, workspace,
                                          workspace_bytes, stream);
    if (rc != KGDET_E_UNSUPPORTED) return rc;
  }
  const int cpdg = s->C / s->deformable_groups;
  const BwdLdsPlan pl = plan_bwd_lds(s, d);
  if (pl.ok && mfma_bwd_ok(s)) {   // (channel tiles that straddle deformable groups: the channel runs of the path below)
    // gather path: no atomics anywhere, outputs need no pre-zeroing
    const size_t need = pl.workspace_bytes();
    if (workspace == nullptr || workspace_bytes < need) {
      set_error("workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
      return KGDET_E_WORKSPACE;
    }
    float *slabs = (float *)workspace;
    float *off_part = slabs + pl.slab_floats;
    float *mask_part = mask ? off_part + pl.off_floats : nullptr;
    int2 *entries = (int2 *)align_up((size_t)(off_part + pl.off_floats + pl.mask_floats), 16);
    int *row_ptr = (int *)(entries + pl.entry_pairs);
    if (int rc = allow_lds<dcn_bwd_input_gather>(kMaxLds)) return rc;
    if (int rc = allow_lds<dcn_bwd_build_index>(kMaxLds - 64)) return rc;
    {
      DcnProblem p;
      fill_problem(s, d, 0, p);
      p.x = input; p.offset = offset; p.mask = mask;
      hipLaunchKernelGGL(dcn_bwd_build_index, dim3(s->N * s->deformable_groups * d.K), dim3(256),
                         pl.index_lds_bytes, (hipStream_t)stream, p, row_ptr, entries);
    }
    for (int g = 0; g < s->groups; ++g) {
      DcnProblem p;
      fill_problem(s, d, g, p);
      p.x = input; p.offset = offset; p.mask = mask;
      p.wpk = packed_weight + weight_images(s, d, g).bwd;
      DcnBwdInputLdsArgs a{};
      a.grad_out = grad_output; a.slabs = slabs; a.off_part = off_part; a.mask_part = mask_part;
      a.Og_pad16 = d.Og_pad16; a.Cg_pad256 = d.Cg_pad256;
      a.n_cslices = pl.n_cslices; a.S = pl.S; a.n_pblocks = pl.n_pblocks; a.slice_base = g * pl.n_cslices;
      a.HWp = pl.HWp;
      hipLaunchKernelGGL(dcn_bwd_input_gather, dim3(pl.n_blocks), dim3(kThreads), pl.lds_bytes, (hipStream_t)stream,
                         p, a, (const int *)row_ptr, (const int2 *)entries);
      hipLaunchKernelGGL(dcn_bwd_input_fixup, dim3(ceil_div(32 * s->H * s->W, 256 * 4), s->N * pl.n_cslices), dim3(256),
                         0, (hipStream_t)stream, p, a, grad_input);
    }
    const long long off_elems = (long long)s->N * s->deformable_groups * 2 * d.K * d.Ho * d.Wo;
    int fix_grid = (int)((off_elems + 255) / 256);
    if (fix_grid > 4096) fix_grid = 4096;
    hipLaunchKernelGGL(dcn_bwd_offset_fixup, dim3(fix_grid), dim3(256), 0, (hipStream_t)stream,
                       (const float *)off_part, (const float *)mask_part, grad_offset, grad_mask, pl.n_slices_total,
                       s->N, s->deformable_groups, d.K, d.Ho * d.Wo, pl.n_cslices, d.Cg, cpdg);
    KGDET_CHECK_LAUNCH("dcn_bwd_input_gather");
    return KGDET_OK;
  }
  // large feature maps, v1 and v2, any weight groups / deformable groups: materialised transposed column gradient + inverse index
  // per CHANNEL RUN (channels that share weight group and deformable group), no atomics (dcn_backward_large.hip).  Rounds 1-4 kept
  // a float-atomic scatter kernel (dcn_bwd_input_mfma) for groups on such maps -- the reference's one non-deterministic piece
  // (deform_conv_cuda_kernel.cu:329) -- and -munsafe-fp-atomics in the Makefile for it: both gone.
  bool seen_dg[64] = {false};
  if (s->deformable_groups > 64) { set_error("more than 64 deformable groups"); return KGDET_E_UNSUPPORTED; }
  std::vector<ChannelRun> runs(channel_runs(s, d, nullptr, 0));   // (any number of them: one launch sequence each)
  channel_runs(s, d, runs.data(), (int)runs.size());
  auto run_problem = [&](const ChannelRun &r) {
    DcnProblem q;
    fill_problem(s, d, r.g, q);
    q.C_total = r.c1 - r.c0; q.mask = mask;
    return q;
  };
  for (const ChannelRun &r : runs)   // eligibility first (nothing launched on failure)
    if (!dcn_bwd_large_ok(run_problem(r), mask != nullptr, 1)) {
      set_error("backward_input on a map of %d pixels: channel run [%d, %d) is not eligible for the column-gradient path "
                "(output channels per group %% 16, (taps x channels) %% 2, at most 49 taps)", s->H * s->W, r.c0, r.c1);
      return KGDET_E_UNSUPPORTED;
    }
  for (const ChannelRun &r : runs) {
    DcnProblem q = run_problem(r);
    q.x = input + (size_t)r.c0 * s->H * s->W; q.offset = offset;
    q.dgi = r.dgi;
    // [K][Cg_pad][Og_pad]: from the run's first channel
    q.wpk = packed_weight + weight_images(s, d, r.g).fwd + (size_t)(r.c0 - r.g * d.Cg) * d.Og_pad;
    if (int rc = dcn_bwd_large(q, grad_output, o_total(s), s->out_channel_offset + r.g * d.Og, grad_input, grad_offset,
                               grad_mask, workspace, workspace_bytes, stream, s->C, r.c0, seen_dg[r.dgi] ? 1 : 0))
      return rc;
    seen_dg[r.dgi] = true;
  }
  return KGDET_OK;
}

int kgdet_deform_conv_backward_weight(const kgdet_dcn_shape *s, const float *input, const float *offset,
                                      const float *mask, const float *grad_output, float *grad_weight,
                                      float *grad_bias, int accumulate, void *workspace, size_t workspace_bytes,
                                      void *stream) {
  Derived d;
  if (int rc = derive(s, d)) return rc;
  KGDET_CHECK_SHAPE(input && offset && grad_output && grad_weight, "null pointer");
  // v1 or v2, any weight / deformable groups: the split-operand kernel with natural-layout output -- small maps on the
  // LDS plane, larger ones gathering from a pixel-major copy of x
  if (!accumulate && g_options[KGDET_OPT_EXACT_BACKWARD] == 0 && (plane_ok(s, d) || gather_ok(s, d))) {
    const int rc = grad_weight_plane_grouped(1, &s, &input, &offset, mask ? &mask : nullptr, &grad_output, &grad_weight, workspace,
                                             workspace_bytes, stream, !plane_ok(s, d));
    if (rc == KGDET_OK) return launch_bias_grad(s, d, grad_output, grad_bias, accumulate, stream);
    // (KGDET_E_WORKSPACE is returned as it is: falling through to the f32 kernel, which needs less, gave a short buffer
    // KGDET_OK with another summation order than the same call on the queried size)
    if (rc != KGDET_E_UNSUPPORTED) return rc;   // else: the f32 kernel below
  }
  const int cpdg = s->C / s->deformable_groups;
  if (!(s->deformable_groups == 1 || cpdg % d.Cg == 0 || (d.Cg % cpdg == 0 && cpdg % kTileN == 0))) {
    set_error("deformable_groups=%d / groups=%d / C=%d: channel tiles straddle deformable groups (unsupported)",
              s->deformable_groups, s->groups, s->C);
    return KGDET_E_UNSUPPORTED;
  }
  const size_t need = slab_bytes() + wgrad_image_bytes(s, d);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    return KGDET_E_WORKSPACE;
  }
  float *slabs = (float *)workspace;
  float *gpk = (float *)((char *)workspace + slab_bytes());  // packed gradient image
  const int G = grid_size();
  for (int g = 0; g < s->groups; ++g) {
    DcnProblem p;
    fill_problem(s, d, g, p);
    p.x = input; p.offset = offset; p.mask = mask;
    p.out = gpk + weight_images(s, d, g).fwd;
    DcnBwdWeightArgs a{};
    a.grad_out = grad_output;
    a.n_ctiles = ceil_div(d.Cg_pad, kTileN);
    a.n_otiles = d.Og_pad / kTileM;
    a.stages_per_tile = ceil_div(p.P, kChunk);
    a.Cg_pad128 = a.n_ctiles * kTileN;
    const int n_tiles = d.K * a.n_otiles * a.n_ctiles;
    a.total_units = (long long)n_tiles * a.stages_per_tile;
    hipLaunchKernelGGL(dcn_bwd_weight_mfma, dim3(G), dim3(kThreads), 0, (hipStream_t)stream, p, a, slabs);
    hipLaunchKernelGGL(dcn_bwd_weight_fixup, dim3(n_tiles, 4), dim3(kThreads), 0, (hipStream_t)stream, p, a,
                       (const float *)slabs, G);
  }
  KGDET_CHECK_LAUNCH("dcn_bwd_weight_mfma");
  if (int rc = kgdet_dcn_unpack_weight_grad(s, gpk, grad_weight, accumulate, stream)) return rc;
  return launch_bias_grad(s, d, grad_output, grad_bias, accumulate, stream);
}

}  // extern "C"
