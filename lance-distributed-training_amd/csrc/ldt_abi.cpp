// ldt_abi.cpp — host side of libldt.so: the C-ABI declared in include/ldt.h.
//
// Per batch the host does planning only, and that is not done here: the
// HIP-free planner (ldt_plan.cpp plan_batch) walks each cell's JPEG marker
// segments (SOI..SOS, a few hundred bytes; the entropy-coded data is never
// touched on the host), dedupes Huffman/quantisation tables, sizes the device
// workspace and lays out one compact plan blob (descriptors, segments, tables,
// the ToTensor/Normalize LUT, labels, per-image status). This file is the
// driver: decode_core starts the cells' copy, has the batch planned while it
// runs, puts the blob into a pinned ring slot and grows the device buffers.
// One H2D copy moves the plan, one moves the cells (unless they are already
// resident), then the kernels run on the caller's stream.
//
// Replaces, per batch: lance_iterable.py:41-49 (to_pylist, PIL open/convert,
// Resize, ToTensor, stack, label tensor) and lance_map_style.py:34-44.
#include <hip/hip_runtime.h>
#include <sched.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/ldt.h"
#include "ldt_blur.hpp"
#include "ldt_augment.hpp"
#include "ldt_color.hpp"
#include "ldt_hostcopy.hpp"
#include "ldt_kernels.hpp"
#include "ldt_plan.hpp"
#include "ldt_resample.hpp"
#include "ldt_sync_cache.hpp"

using namespace ldt;

// ---------------------------------------------------------------------------
// Context.
// ---------------------------------------------------------------------------
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
};

struct PinBuf {
  void *p = nullptr;
  size_t cap = 0;
};

// Host phases of decode_core (LDT_OPT_HOST_TIMING; read with ldt_host_times).
enum HostPhase {
  kHpSlot = 0, // waiting for the pinned slot, starting the cell copy
  kHpParse,    // plan_batch: header walk + per-image plans (overlaps the cell copy)
  kHpPlan,     // plan blob, device workspace sizing
  kHpCopy,     // waiting for the cell copy to finish, H2D enqueue
  kHpLaunch,   // kernel launches
  kHpStatus,   // status copy, return
  // not phases of the calling thread: the copy pool's wake-up (copy start to
  // the first chunk a pool thread took) and span (copy start to its end)
  kHpCopyWake,
  kHpCopySpan,
  kHpCount
};

#ifndef LDT_FUSE_DEFAULT
#define LDT_FUSE_DEFAULT true // experiment builds: -DLDT_FUSE_DEFAULT=false
#endif

// The per-call options a context holds for its next decode / resize call.
// crops / windows: one row per (image, view), image-major; colors / augs: one
// entry per output image (colours validated when they are set, augments'
// ranges too, what depends on the output size by the decode call);
// view_sizes: (h, w) per view, empty = none; views: 1 = none pending;
// drafts: one libjpeg scale (1, 2, 4 or 8) per row, validated when set.
struct PendingCall {
  std::vector<ldt_crop> crops;
  std::vector<ldt_window> windows;
  std::vector<ldt_color> colors;
  std::vector<ldt_aug> augs;
  std::vector<int32_t> view_sizes;
  std::vector<int32_t> drafts;
  // mixes: one record per row (ldt_set_mix), with the call's class count and
  // the device buffer of its soft labels
  std::vector<ldt_mix> mixes;
  int32_t mix_classes = 0;
  float *mix_soft = nullptr;
  int views = 1;
  bool boxed = false, windowed = false, colored = false, augmented = false, mixed = false, drafted = false;
};

struct ldt_ctx {
  int device = 0;
  std::string err;
  bool sync_status = true;
  int huff_mode = 0;
  int resize_impl = 0;
  int warm_pct = 0;
  int subseq_bits = 256; // minimum S of the parallel decoder
  int resize_waves_pct = 100;
  int resize_wpg = 0;
  bool fuse_destuff = LDT_FUSE_DEFAULT; // LDT_OPT_FUSED_DESTUFF
  int copy_threads = -1; // -1: default (from the cgroup quota per local rank, <= 6)
  int copy_bind = 2;      // LDT_OPT_COPY_BIND: pool threads on GPU-local cores' L3 domains (1: the cores)
  bool copy_nt = true;    // LDT_OPT_COPY_NT: non-temporal stores into the slot
  int copy_mode = 0;      // LDT_OPT_COPY_MODE: 0 DMA on the device's copy stream, 1 on the caller's
  hipStream_t copy_stream = nullptr; // ldt_set_copy_stream: replaces the device's copy stream (mode 0)
  bool host_timing = false;
  bool debug_counters = false; // LDT_OPT_DEBUG_COUNTERS
  int sync_cache = 1;          // LDT_OPT_SYNC_CACHE (the table is the device's: sc_view)
  int64_t win_cap = -1;        // LDT_OPT_HUFF_WINDOW: cap on k_huff_image's LDS window (bytes; -1 none)
  CopyPlacement placement; // of the current pool
  static constexpr int kSlots = 2;
  // device cells, one buffer per pinned slot: a copy-stream DMA into one may
  // run while the kernels of the slot's previous batch still read the other
  DevBuf d_data[kSlots];
  hipEvent_t data_free_ev[kSlots] = {nullptr, nullptr}; // its last reader (Huffman stage) done
  hipEvent_t h2d_ev[kSlots] = {nullptr, nullptr};       // its DMA done (copy stream)
  bool data_used[kSlots] = {false, false};
  DevBuf d_plan, d_dstuf, d_coef, d_brec, d_bcarry, d_pcoef, d_dcv, d_planes, d_raw, d_dscnt;
  DevBuf d_perm; // DistributedSampler scratch: 3 int32 arrays of dataset_len
  std::unique_ptr<CopyPool> copier; // host -> pinned copies (created on first use)
  PinBuf h_data[kSlots], h_plan[kSlots];
  hipEvent_t slot_ev[kSlots] = {nullptr, nullptr};
  bool slot_used[kSlots] = {false, false};
  int slot = 0;
  // per-image status of the last decode on each pinned slot (device part,
  // copied back at the end of the batch): ticket = the call's number, event
  // = recorded after the copy, so a status can be read `kSlots` calls later
  // without waiting for the newer batches (ldt_fetch_status_ticket)
  int32_t *h_status[kSlots] = {nullptr, nullptr}; // pinned
  size_t h_status_cap[kSlots] = {0, 0};
  hipEvent_t st_ev[kSlots] = {nullptr, nullptr};
  int64_t st_ticket[kSlots] = {-1, -1};
  int64_t st_n[kSlots] = {0, 0};
  int64_t tickets = 0; // decode calls that enqueued work
  int last_sl = 0;     // slot of the most recent decode
  int64_t last_n = 0;
  hipEvent_t done_ev = nullptr;
  hipStream_t last_stream = nullptr;
  bool have_last = false;
  // the progressive coefficient buffer must be all zero between batches
  // (k_idct restores it); set while k_prog output may be in it without a
  // k_idct launched after it, so the next call clears it
  bool coef_dirty = false;
  HuffCache huff; // baseline Huffman tables derived so far (plan_batch)
  // Pillow resample coefficient tables of the input sizes seen so far, which
  // k_resize4 loads (ldt_types.hpp kResamp*): kResampTableBytes of HBM,
  // allocated with the first resize and never moved or shrunk, so entries are
  // added while earlier batches' kernels read theirs. resamp_have[size]: not
  // zero once the entry's fill is enqueued on a stream that every later call
  // is ordered after (order_streams), and then the entry's real tap count
  // (resample_taps_host, computed once with the fill).
  DevBuf d_resamp;
  std::vector<uint8_t> resamp_have;
  int64_t resamp_fills = 0; // k_fill_resample launches (ldt_debug_resample_fills)
  // The output size (ldt_set_output_size) every decode / resize call reads
  // when it is made; the kernels get it by value, so a later change never
  // touches a batch in flight.
  int out_h = kOut, out_w = kOut;
  // The resize's filter (ldt_set_filter), read like the output size: by every
  // decode / resize call when it is made, which hands it to its kernel as a
  // template argument, so a later change never touches a batch in flight.
  int filter = kFilterBilinear;
  // The output's element type and layout (ldt_set_output_format), read like
  // the filter: by every decode / resize call when it is made, which passes
  // it to its kernels by value.
  OutFmt fmt;
  // What the next decode / ldt_resize_raw call was handed (ldt_set_crops,
  // _windows, _views, _view_sizes, _colors, _augments, _mix, _draft): that call takes it out
  // of the context first thing (take_pending), whatever becomes of it.
  PendingCall pending;
  int view_order = 0; // LDT_OPT_VIEW_ORDER
  // The photometric stage's device buffers, grown on demand: the call's
  // entries, one L counter per entry, and the resized bytes the resize writes
  // for the two colour kernels to read. h_color: the entries' pinned staging,
  // one per slot like the plan's.
  DevBuf d_color, d_colsum, d_colws;
  PinBuf h_color[kSlots];
  // The auto-augment stage resizes into d_colws too; d_augws: the second
  // workspace its ops ping-pong with, d_aug: the entries, d_augstat:
  // kAugStatBytes per entry, h_aug: the pinned staging.
  DevBuf d_aug, d_augstat, d_augws;
  PinBuf h_aug[kSlots];
  // The mix stage reads d_colws, or d_augws when a colour or augment stage
  // ran before it; d_mix: the float32 ToTensor / Normalize table (kMixLutBytes)
  // followed by the call's records, h_mix: the pinned staging of both.
  DevBuf d_mix;
  PinBuf h_mix[kSlots];
  // Tables for an output size other than kOut: [0] horizontal (rows of
  // resamp_g_out[0] = out_w entries, kResampTableBytesH), [1] vertical (out_h,
  // kResampTableBytesV). Allocated when first needed, never moved; a size
  // change resets the axis' `have` flags, and the refill runs on the next
  // batch's stream, which order_streams puts behind every earlier reader.
  DevBuf d_resamp_g[2];
  std::vector<uint8_t> resamp_g_have[2];
  int resamp_g_out[2] = {0, 0};
  // stage profiling: one event per stage boundary, sets recycled once read
  bool profile = false;
  struct EvSet {
    hipEvent_t ev[LDT_NUM_STAGES + 1];
    int first_stage, last_stage; // stages [first, last) were recorded
  };
  std::vector<EvSet> ev_free, ev_pending;
  double stage_ms[LDT_NUM_STAGES] = {};
  int64_t stage_cnt[LDT_NUM_STAGES] = {};
  EvSet *cur_ev = nullptr;
  int64_t last_off_redo = -1; // debug counters of the last batch (plan blob offset)
  int last_resize_wpg = -1;   // k_resize4 waves per workgroup of the last batch, JPEG or raw (0: streaming kernel)
  int last_resize_bands = 0;  // that batch's k_resize4 bands per image (ldt_debug_last_resize_bands)
  int last_idct_scaled = -1;  // set by launch_idct where it launches: 1 k_idct_scaled, 0 k_idct (ldt_debug_last_idct)
  uint8_t *last_plan_dev = nullptr; // that batch's plan blob on the device
  double host_us[kHpCount] = {};
  int64_t host_calls = 0;
};

namespace {

// Host phase times of decode_core (LDT_OPT_HOST_TIMING = 1), accumulated per
// context and read with ldt_host_times. Diagnostic only.
struct HostTimer {
  ldt_ctx *c;
  bool on;
  std::chrono::steady_clock::time_point t;
  explicit HostTimer(ldt_ctx *cc) : c(cc), on(cc->host_timing) {
    if (on) t = std::chrono::steady_clock::now();
  }
  void mark(int k) {
    if (!on) return;
    const auto n = std::chrono::steady_clock::now();
    c->host_us[k] += std::chrono::duration<double, std::micro>(n - t).count();
    t = n;
    if (k == kHpStatus) ++c->host_calls;
  }
};

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

int set_err(ldt_ctx *c, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

#define HIPCHK(ctx, expr)                                                                      \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return set_err(ctx, LDT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));         \
  } while (0)

// Grow a device buffer; contents are not preserved (a new allocation is
// zero-filled on `s` when `zero`). Synchronises `s` first so no in-flight work
// still references the old allocation.
int ensure_dev(ldt_ctx *c, DevBuf &b, size_t need, hipStream_t s, bool zero = false) {
  if (b.cap >= need) return LDT_OK;
  size_t cap = need + need / 4 + 4096;
  if (b.p) {
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipDeviceSynchronize());
    // the last batch's plan blob (ldt_debug_counters) may live in this buffer
    const uintptr_t lo = (uintptr_t)b.p, lp = (uintptr_t)c->last_plan_dev;
    if (lp >= lo && lp < lo + b.cap) {
      c->last_plan_dev = nullptr;
      c->last_off_redo = -1;
    }
    HIPCHK(c, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
  }
  if (hipMalloc(&b.p, cap) != hipSuccess)
    return set_err(c, LDT_ERR_NOMEM, "hipMalloc(%zu) failed", cap);
  b.cap = cap;
  if (zero) HIPCHK(c, hipMemsetAsync(b.p, 0, cap, s));
  return LDT_OK;
}

// Host ranges page-locked in place (ldt_register_host), for all contexts. A
// decode that DMAs from a range holds it (inflight) until its copy is
// enqueued and marks the device it used; ldt_unregister_host drops the range,
// waits for the holders, then synchronises every device that used it before
// unpinning.
struct HostRange {
  uintptr_t lo, hi;
  int inflight = 0;
  uint64_t devmask = 0;
};
std::mutex g_host_m;
std::condition_variable g_host_cv;
std::vector<std::shared_ptr<HostRange>> g_host_ranges;

std::shared_ptr<HostRange> host_acquire(const void *p, size_t n, int dev) {
  const uintptr_t lo = (uintptr_t)p, hi = lo + n;
  std::lock_guard<std::mutex> l(g_host_m);
  for (auto &r : g_host_ranges)
    if (lo >= r->lo && hi <= r->hi) {
      ++r->inflight;
      r->devmask |= 1ull << (dev & 63);
      return r;
    }
  return nullptr;
}

void host_release(std::shared_ptr<HostRange> &r) {
  if (!r) return;
  {
    std::lock_guard<std::mutex> l(g_host_m);
    --r->inflight;
  }
  g_host_cv.notify_all();
  r.reset();
}

bool host_registered(const void *p, size_t n) {
  const uintptr_t lo = (uintptr_t)p, hi = lo + n;
  std::lock_guard<std::mutex> l(g_host_m);
  for (const auto &r : g_host_ranges)
    if (lo >= r->lo && hi <= r->hi) return true;
  return false;
}

CopyPool &copier(ldt_ctx *c) {
  if (!c->copier) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), c->device) != hipSuccess) {
      (void)hipGetLastError();
      bus[0] = 0;
    }
    c->placement = copy_placement(bus, c->copy_threads, c->copy_bind != 0);
    c->copier.reset(new CopyPool(c->placement.cpus, c->copy_nt, c->copy_bind == 2));
  }
  return *c->copier;
}

void pinned_copy(ldt_ctx *c, void *dst, const void *src, size_t n) {
  CopyPool &p = copier(c);
  p.start(dst, src, n);
  p.finish();
}

// The device's sync cache (ldt_sync_cache.hpp): one table per
// device, shared by the process's contexts (the pipeline's slot contexts keep
// no copies), allocated whole by the first decode that uses it and freed
// with the device's last context. `failed`: the allocation did not fit; the
// device then decodes without the table until the budget changes.
struct ScTable {
  void *p = nullptr;
  int64_t sets = 0;
  int64_t budget_mb = 1024;
  int ctxs = 0;
  bool failed = false;
};
std::mutex g_sc_m;
ScTable g_sc[64];

void sc_free_locked(ScTable &t) {
  if (t.p) {
    (void)hipDeviceSynchronize(); // launches that carry the pointer
    (void)hipFree(t.p);
  }
  t.p = nullptr;
  t.sets = 0;
  t.failed = false;
}

// The view a decode on `s` hands k_huff_image (sets 0: off).
ScView sc_view(ldt_ctx *c, hipStream_t s) {
  ScView v;
  if (c->sync_cache == 0 || c->debug_counters || c->device < 0 || c->device >= 64) return v;
  std::lock_guard<std::mutex> l(g_sc_m);
  ScTable &t = g_sc[c->device];
  if (!t.p && !t.failed) {
    const int64_t sets = sc_sets(t.budget_mb << 20);
    if (sets == 0) {
      t.failed = true;
    } else if (hipMalloc(&t.p, (size_t)sc_table_bytes(sets)) != hipSuccess ||
               hipMemsetAsync(t.p, 0, (size_t)sc_off_payloads(sets), s) != hipSuccess ||
               hipStreamSynchronize(s) != hipSuccess) {
      (void)hipGetLastError();
      if (t.p) (void)hipFree(t.p);
      t.p = nullptr;
      t.failed = true;
    } else {
      t.sets = sets;
    }
  }
  if (!t.p) return v;
  v.base = static_cast<uint8_t *>(t.p);
  v.sets = (int32_t)t.sets;
  v.stats = c->sync_cache == 2;
  return v;
}

// One non-blocking stream per device for the cells' H2D DMA (LDT_OPT_COPY_MODE
// 0), shared by the process's contexts: the transfer of a batch then runs
// while the kernels of the batches before it still occupy the contexts'
// streams (one more HIP stream per process; the copy engine does the work).
hipStream_t copy_stream(int device) {
  static std::mutex m;
  static hipStream_t streams[64] = {};
  std::lock_guard<std::mutex> l(m);
  if (device < 0 || device >= 64) return nullptr;
  if (!streams[device] && hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    streams[device] = nullptr;
  }
  return streams[device];
}

// Joins an asynchronous cell copy on every exit path of decode_core: the
// caller's host buffer is borrowed only for the duration of the call.
struct CopyJoin {
  CopyPool *p = nullptr;
  void wait() {
    if (p) p->finish();
    p = nullptr;
  }
  ~CopyJoin() { wait(); }
};

int ensure_pin(ldt_ctx *c, PinBuf &b, size_t need) {
  if (b.cap >= need) return LDT_OK;
  size_t cap = need + need / 4 + 4096;
  if (b.p) {
    HIPCHK(c, hipHostFree(b.p));
    b.p = nullptr;
    b.cap = 0;
  }
  if (hipHostMalloc(&b.p, cap, hipHostMallocDefault) != hipSuccess)
    return set_err(c, LDT_ERR_NOMEM, "hipHostMalloc(%zu) failed", cap);
  b.cap = cap;
  return LDT_OK;
}

// Grow pinned slot `sl`'s buffer (`which` = h_data or h_plan) and, while it
// is idle, the other slot's to the same size: a pinned allocation costs
// milliseconds, so it should not wait for the first call on the other slot.
int ensure_pin_slots(ldt_ctx *c, PinBuf (&bufs)[ldt_ctx::kSlots], int sl, size_t need) {
  int rc;
  if ((rc = ensure_pin(c, bufs[sl], need))) return rc;
  for (int k = 0; k < ldt_ctx::kSlots; ++k) {
    if (k == sl || bufs[k].cap >= need) continue;
    if (c->slot_used[k] && hipEventQuery(c->slot_ev[k]) != hipSuccess) continue;
    (void)hipGetLastError();
    if ((rc = ensure_pin(c, bufs[k], need))) return rc;
  }
  return LDT_OK;
}

// Wait until the pinned slot's previous H2D copies have completed.
int acquire_slot(ldt_ctx *c) {
  c->slot = (c->slot + 1) % ldt_ctx::kSlots;
  if (c->slot_used[c->slot]) HIPCHK(c, hipEventSynchronize(c->slot_ev[c->slot]));
  return LDT_OK;
}

// Order this call after the previous one when the caller switches streams.
int order_streams(ldt_ctx *c, hipStream_t s) {
  if (c->have_last && c->last_stream != s) HIPCHK(c, hipStreamWaitEvent(s, c->done_ev, 0));
  return LDT_OK;
}

// The pending options, taken out of the context, which then holds none.
PendingCall take_pending(ldt_ctx *c) { return std::exchange(c->pending, PendingCall{}); }

int finish_call(ldt_ctx *c, hipStream_t s) {
  HIPCHK(c, hipEventRecord(c->done_ev, s));
  c->last_stream = s;
  c->have_last = true;
  return LDT_OK;
}

// ---- stage profiling helpers ----
void prof_begin(ldt_ctx *c, int first_stage, hipStream_t s) {
  c->cur_ev = nullptr;
  if (!c->profile) return;
  ldt_ctx::EvSet es;
  if (!c->ev_free.empty()) {
    es = c->ev_free.back();
    c->ev_free.pop_back();
  } else {
    for (int k = 0; k <= LDT_NUM_STAGES; ++k)
      if (hipEventCreate(&es.ev[k]) != hipSuccess) return;
  }
  es.first_stage = es.last_stage = first_stage;
  c->ev_pending.push_back(es);
  c->cur_ev = &c->ev_pending.back();
  (void)hipEventRecord(c->cur_ev->ev[first_stage], s);
}

// Marks the end of `stage` (events for stages must be recorded in order).
void prof_mark(ldt_ctx *c, int stage, hipStream_t s) {
  if (!c->cur_ev) return;
  (void)hipEventRecord(c->cur_ev->ev[stage + 1], s);
  c->cur_ev->last_stage = stage + 1;
}

// The batch's cells (pinned slot or registered pages) -> the slot's device
// buffer. LDT_OPT_COPY_MODE 0: one DMA on the device's copy stream, after the
// kernels that last read that buffer; `s` waits for it. Mode 1 (or no copy
// stream): on `s` itself, behind the previous batch's kernels.
int enqueue_cells(ldt_ctx *c, int sl, const void *src, size_t n, hipStream_t s) {
  hipStream_t cs = c->copy_mode != 0 ? nullptr : (c->copy_stream ? c->copy_stream : copy_stream(c->device));
  if (!cs) {
    HIPCHK(c, hipMemcpyAsync(c->d_data[sl].p, src, n, hipMemcpyHostToDevice, s));
    return LDT_OK;
  }
  if (c->data_used[sl]) HIPCHK(c, hipStreamWaitEvent(cs, c->data_free_ev[sl], 0));
  HIPCHK(c, hipMemcpyAsync(c->d_data[sl].p, src, n, hipMemcpyHostToDevice, cs));
  HIPCHK(c, hipEventRecord(c->h2d_ev[sl], cs));
  HIPCHK(c, hipStreamWaitEvent(s, c->h2d_ev[sl], 0));
  return LDT_OK;
}

// The context's resample coefficient cache: collects the sizes whose entries
// of one table are missing and fills them on `s`, up to kResampFill sizes per
// launch. Sizes without an entry (resamp_cached: past the table's input limit
// or with more taps than a row's) are left out: k_resize4 computes such an
// image's vertical coefficients itself, and a batch with such a width takes
// the streaming kernel.
struct ResampFill {
  ldt_ctx *c;
  hipStream_t s;
  int32_t *tab;
  int out, max_in;
  std::vector<uint8_t> &have;
  ResampSizes sz{};
  int add(int size) {
    if (!resamp_cached(size, out, max_in) || have[size]) return LDT_OK;
    have[size] = (uint8_t)resample_taps_host(size, out); // >= 1: the entry exists, and its real tap count
    sz.size[sz.n++] = (uint16_t)size;
    return sz.n == kResampFill ? flush() : LDT_OK;
  }
  int flush() {
    if (sz.n == 0) return LDT_OK;
    const hipError_t e = launch_fill_resample(sz, tab, out, s);
    if (e != hipSuccess)
      for (int i = 0; i < sz.n; ++i) have[sz.size[i]] = 0;
    sz.n = 0;
    HIPCHK(c, e);
    ++c->resamp_fills;
    return LDT_OK;
  }
};

// The table that serves output size `out` on `axis` (0 horizontal, 1
// vertical), allocated on first use: the kOut table, or the axis' table for
// the context's current size, reset when that size changed.
int resamp_table(ldt_ctx *c, int out, int axis, DevBuf **buf, std::vector<uint8_t> **have, int *max_in) {
  if (out == kOut) {
    if (!c->d_resamp.p) {
      if (hipMalloc(&c->d_resamp.p, kResampTableBytes) != hipSuccess)
        return set_err(c, LDT_ERR_NOMEM, "hipMalloc(%zu) failed", kResampTableBytes);
      c->d_resamp.cap = kResampTableBytes;
      c->resamp_have.assign(kResampMaxSize + 1, 0);
    }
    *buf = &c->d_resamp;
    *have = &c->resamp_have;
    *max_in = kResampMaxSize;
    return LDT_OK;
  }
  const size_t bytes = axis == 0 ? kResampTableBytesH : kResampTableBytesV;
  DevBuf &b = c->d_resamp_g[axis];
  if (!b.p) {
    if (hipMalloc(&b.p, bytes) != hipSuccess) return set_err(c, LDT_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    b.cap = bytes;
  }
  if (c->resamp_g_out[axis] != out) {
    c->resamp_g_have[axis].assign(kResampMaxSize + 1, 0);
    c->resamp_g_out[axis] = out;
  }
  *buf = &b;
  *have = &c->resamp_g_have[axis];
  *max_in = resamp_max_in(out, bytes);
  return LDT_OK;
}

// The tables of the context's output size with the entries of `sizes` (input
// widths for axis 0, heights for axis 1) filled on `s`. Outputs wider than
// kTileCols take the streaming kernel, which computes its own coefficients:
// no tables then (ro.tab_h stays null).
template <typename Sizes>
int resize_tables(ldt_ctx *c, hipStream_t s, const Sizes &widths, const Sizes &heights, ResizeOut &ro) {
  ro.oh = c->out_h;
  ro.ow = c->out_w;
  ro.generic = c->resize_impl == 3;
  if (c->resize_impl == 2 || ro.ow > kTileCols) return LDT_OK;
  int rc;
  for (int axis = 0; axis < 2; ++axis) {
    DevBuf *buf;
    std::vector<uint8_t> *have;
    int max_in;
    if ((rc = resamp_table(c, axis ? ro.oh : ro.ow, axis, &buf, &have, &max_in))) return rc;
    ResampFill rf{c, s, static_cast<int32_t *>(buf->p), axis ? ro.oh : ro.ow, max_in, *have};
    for (int v : (axis ? heights : widths))
      if ((rc = rf.add(v))) return rc;
    // a square size at kOut shares one table: the other axis' sizes too
    if (ro.oh == ro.ow && ro.oh == kOut)
      for (int v : (axis ? widths : heights))
        if ((rc = rf.add(v))) return rc;
    if ((rc = rf.flush())) return rc;
    (axis ? ro.tab_v : ro.tab_h) = static_cast<const int32_t *>(buf->p);
    (axis ? ro.max_in_v : ro.max_in_h) = max_in;
    // the batch's taps on this axis: the most of any of its sizes, which need
    // not be the largest size's
    int taps = 1;
    for (int v : (axis ? heights : widths))
      taps = std::max(taps, resamp_cached(v, rf.out, max_in) ? (int)(*have)[v] : resample_ksize_host(v, rf.out));
    (axis ? ro.taps_v : ro.taps_h) = taps;
  }
  return LDT_OK;
}

// What check_call makes of a decode call's pending options.
constexpr size_t kMixLutBytes = 768 * sizeof(float); // the float32 table ahead of a call's mix records

struct CallShape {
  int views = 1;             // views per image: the pending ones, or the size list's length
  bool sized = false;        // the call has per-view sizes
  int32_t hw[2 * kMaxViews]; // (h, w) of every view's output (a call with colours or augments)
  ColorGeom cgeom;           // that call's colour / augment kernel geometry
  int aug_k = 0;             // the largest count among the augments: the stage's slots
};

// A decode call's arguments and pending options `pc` against each other and
// the context's settings, before anything is enqueued or allocated; fills
// `cs`. `ptrs_ok`: the call's pointers serve n rows. `labels`: the rows' own
// (host), or null: a mix with classes needs each in its range.
int check_call(ldt_ctx *c, const PendingCall &pc, int64_t n, bool ptrs_ok, const ldt_norm *norm, CallShape &cs,
               const int64_t *labels = nullptr) {
  const std::vector<ldt_crop> &crops = pc.crops;
  const std::vector<ldt_window> &windows = pc.windows;
  const std::vector<int32_t> &vsz = pc.view_sizes;
  const std::vector<ldt_aug> &augs = pc.augs;
  const bool boxed = pc.boxed, windowed = pc.windowed;
  const bool sized = cs.sized = !vsz.empty();
  int &views = cs.views = pc.views;
  if (n < 0 || !ptrs_ok) return set_err(c, LDT_ERR_ARG, "bad argument (n=%lld)", (long long)n);
  if (pc.drafted && (int64_t)pc.drafts.size() != n)
    return set_err(c, LDT_ERR_ARG, "draft scales for %lld rows, the batch has %lld", (long long)pc.drafts.size(),
                   (long long)n);
  if (sized) {
    // the sizes imply the views; views pending with another count contradict them
    const int sv = (int)(vsz.size() / 2);
    if (views != 1 && views != sv)
      return set_err(c, LDT_ERR_ARG, "%d views pending (ldt_set_views) with %d view sizes (ldt_set_view_sizes)", views,
                     sv);
    views = sv;
  }
  if (views == 1 && !sized) {
    if (boxed && (int64_t)crops.size() != n)
      return set_err(c, LDT_ERR_ARG, "crops for %lld rows, the batch has %lld", (long long)crops.size(), (long long)n);
    if (windowed && (int64_t)windows.size() != n)
      return set_err(c, LDT_ERR_ARG, "windows for %lld rows, the batch has %lld", (long long)windows.size(),
                     (long long)n);
  } else {
    // image-major: row i, view v at i * views + v
    if (boxed && (int64_t)crops.size() != n * views)
      return set_err(c, LDT_ERR_ARG, "crops for %lld rows, the batch has %lld rows of %d views",
                     (long long)crops.size(), (long long)n, views);
    if (windowed && (int64_t)windows.size() != n * views)
      return set_err(c, LDT_ERR_ARG, "windows for %lld rows, the batch has %lld rows of %d views",
                     (long long)windows.size(), (long long)n, views);
    // the grid of k_resize_views and the view table's index are ints
    ViewGeomTab geom;
    if (sized ? !view_geom_build(n, views, vsz.data(), kMaxOut, geom)
              : (n > 0x7FFFFFFF / views || resize_views_groups((int)n, views, c->out_h, c->out_w) > 0x7FFFFFFF))
      return set_err(c, LDT_ERR_ARG, "%lld rows of %d views%s: more workgroups than a launch takes", (long long)n,
                     views, sized ? " with their own sizes" : "");
  }
  if (c->fmt.dtype == kDtypeU8 && norm)
    return set_err(c, LDT_ERR_ARG, "a uint8 output (LDT_DTYPE_U8) is the resized byte itself: Normalize cannot apply");
  if (pc.colored && pc.augmented)
    return set_err(c, LDT_ERR_ARG, "colours (ldt_set_colors) and augments (ldt_set_augments) are pending for the same "
                                   "call: the two stages do not compose");
  if (pc.mixed) {
    if ((int64_t)pc.mixes.size() != n)
      return set_err(c, LDT_ERR_ARG, "mix for %lld rows, the batch has %lld", (long long)pc.mixes.size(), (long long)n);
    if (views != 1 || sized)
      return set_err(c, LDT_ERR_ARG, "a mix (ldt_set_mix) with views or a size list pending: the mix stage serves "
                                     "single-view calls only");
    if (c->fmt.dtype == kDtypeU8)
      return set_err(c, LDT_ERR_ARG, "a mix (ldt_set_mix) with a uint8 output (LDT_DTYPE_U8): the mix is float32 "
                                     "arithmetic on the table's values");
    for (size_t i = 0; i < pc.mixes.size(); ++i) {
      const ldt_mix &m = pc.mixes[i];
      if (m.box[2] != 0 && ((int64_t)m.box[0] + m.box[2] > c->out_h || (int64_t)m.box[1] + m.box[3] > c->out_w))
        return set_err(c, LDT_ERR_ARG, "mix row %lld: the box leaves the %d x %d output image", (long long)i,
                       c->out_h, c->out_w);
    }
    if (pc.mix_classes > 0) {
      if (!labels)
        return set_err(c, LDT_ERR_ARG, "a mix with num_classes=%d (ldt_set_mix) and a call without labels",
                       (int)pc.mix_classes);
      for (int64_t i = 0; i < n; ++i)
        if (labels[i] < 0 || labels[i] >= pc.mix_classes)
          return set_err(c, LDT_ERR_ARG, "mix: row %lld has label %lld, outside 0..%d", (long long)i,
                         (long long)labels[i], (int)pc.mix_classes - 1);
    }
  }
  if (!pc.colored && !pc.augmented && !pc.mixed) return LDT_OK;
  // one entry per output image; the stage's kernel geometry
  const int64_t entries = pc.colored ? (int64_t)pc.colors.size() : (int64_t)augs.size();
  if ((pc.colored || pc.augmented) && entries != n * views)
    return set_err(c, LDT_ERR_ARG, "%s for %lld output images, the batch has %lld rows of %d views",
                   pc.colored ? "colours" : "augments", (long long)entries, (long long)n, views);
  int32_t(&hw)[2 * kMaxViews] = cs.hw;
  for (int v = 0; v < views; ++v) {
    hw[2 * v] = sized ? vsz[2 * (size_t)v] : c->out_h;
    hw[2 * v + 1] = sized ? vsz[2 * (size_t)v + 1] : c->out_w;
  }
  if (!color_geom_build(n, views, hw, cs.cgeom))
    return set_err(c, LDT_ERR_ARG, "%lld rows of %d views with %s: more workgroups than a launch takes", (long long)n,
                   views, pc.colored ? "colours" : pc.augmented ? "augments" : "a mix");
  for (size_t i = 0; i < augs.size(); ++i) {
    const ldt_aug &e = augs[i];
    const int oh = hw[2 * (i % views)], ow = hw[2 * (i % views) + 1];
    if (e.erase[2] != 0 && ((int64_t)e.erase[0] + e.erase[2] > oh || (int64_t)e.erase[1] + e.erase[3] > ow))
      return set_err(c, LDT_ERR_ARG, "augment entry %lld: the erase box leaves its %d x %d output image", (long long)i,
                     oh, ow);
    for (int k = 0; k < e.count; ++k)
      if (e.op[k].code == LDT_AUG_AFFINE && !aug_affine_walk_ok(e.op[k].a, ow, oh))
        return set_err(c, LDT_ERR_ARG, "augment entry %lld: op %d's fixed-point walk over %d x %d leaves int32",
                       (long long)i, k, oh, ow);
    cs.aug_k = std::max(cs.aug_k, (int)e.count);
  }
  return LDT_OK;
}

// A staged call's entries (colours or augments) on their way to the device:
// the device buffer and the slot's pinned staging sized, the entries in the
// staging. The copy itself is enqueued later, with the plan's (h2d).
struct StagedEntries {
  void *dev = nullptr;
  const void *pin = nullptr;
  size_t bytes = 0;
  hipError_t h2d(hipStream_t s) const { return hipMemcpyAsync(dev, pin, bytes, hipMemcpyHostToDevice, s); }
};
template <typename E>
int stage_entries(ldt_ctx *c, const std::vector<E> &entries, DevBuf &d, PinBuf (&h)[ldt_ctx::kSlots], int sl,
                  hipStream_t s, StagedEntries &st) {
  int rc;
  st.bytes = entries.size() * sizeof(E);
  if ((rc = ensure_dev(c, d, st.bytes, s))) return rc;
  if ((rc = ensure_pin_slots(c, h, sl, st.bytes))) return rc;
  memcpy(h[sl].p, entries.data(), st.bytes);
  st.dev = d.p;
  st.pin = h[sl].p;
  return LDT_OK;
}

// The photometric stage of a call with colours: what its entries ask for.
struct ColorStage {
  bool mean = false;   // some entry has contrast: the mean pass runs
  int blur_max_r = -1; // some entry has a blur: its largest box radius, and k_color_blur runs
  BlurGeom bgeom;
};

// Workspace -> the call's output. Failed rows are skipped by the kernels and
// zeroed afterwards (staged_tail).
int color_stage(ldt_ctx *c, const ColorStage &st, size_t entries, const DevPlan &p, const DevWork &w, float *out_img,
                OutFmt fmt, const ColorGeom &cgeom, hipStream_t s) {
  const ldt_color *dcol = static_cast<const ldt_color *>(c->d_color.p);
  uint32_t *dsum = static_cast<uint32_t *>(c->d_colsum.p);
  const uint8_t *dws = static_cast<const uint8_t *>(c->d_colws.p);
  if (st.mean) {
    HIPCHK(c, hipMemsetAsync(dsum, 0, 4 * entries, s));
    HIPCHK(c, launch_color_mean(dcol, dws, dsum, w.status, p.n, cgeom, s));
  }
  HIPCHK(c, launch_color_apply(dcol, dws, dsum, w.status, p.lut, out_img, fmt, p.n, cgeom, s));
  if (st.blur_max_r >= 0)
    HIPCHK(c, launch_color_blur(dcol, dws, dsum, w.status, p.lut, out_img, fmt, p.n, st.bgeom, st.blur_max_r, s));
  return LDT_OK;
}

// The auto-augment stage: workspace -> the call's output in max(K, 1) slots;
// stats[slot]: some entry's op in that slot needs the statistics pass. Failed
// rows as in color_stage.
// `to_ws` (a call with a mix): every slot, the last too, writes uint8 planes to
// the other workspace (launch_aug_apply), and K = 0 launches nothing.
int augment_stage(ldt_ctx *c, int aug_k, const bool (&stats)[LDT_MAX_AUG_OPS], const DevPlan &p, const DevWork &w,
                  float *out_img, OutFmt fmt, const ColorGeom &cgeom, hipStream_t s, bool to_ws = false) {
  const ldt_aug *daug = static_cast<const ldt_aug *>(c->d_aug.p);
  uint8_t *dst = static_cast<uint8_t *>(c->d_augstat.p);
  uint8_t *wsa = static_cast<uint8_t *>(c->d_colws.p);
  uint8_t *wsb = aug_k > 1 || (to_ws && aug_k > 0) ? static_cast<uint8_t *>(c->d_augws.p) : wsa; // one slot: never written
  if (to_ws && aug_k == 0) return LDT_OK;
  for (int slot = 0; slot < std::max(aug_k, 1); ++slot) {
    if (aug_k > 0 && stats[slot]) HIPCHK(c, launch_aug_stats(daug, wsa, wsb, dst, w.status, p.n, cgeom, slot, aug_k, s));
    HIPCHK(c, launch_aug_apply(daug, wsa, wsb, dst, w.status, p.lut, out_img, fmt, p.n, cgeom, slot, aug_k, s, to_ws));
  }
  return LDT_OK;
}

// The mix stage: the rows' final uint8 planes -> the call's output, and the
// soft labels when the mix has classes.
int mix_stage(ldt_ctx *c, const PendingCall &pc, bool colored, bool augmented, const DevPlan &p, const DevWork &w,
              float *out_img, OutFmt fmt, const ColorGeom &cgeom, hipStream_t s) {
  const uint8_t *dm = static_cast<const uint8_t *>(c->d_mix.p);
  const float *lut = reinterpret_cast<const float *>(dm);
  const ldt_mix *dmix = reinterpret_cast<const ldt_mix *>(dm + kMixLutBytes);
  const uint8_t *wsa = static_cast<const uint8_t *>(c->d_colws.p);
  const uint8_t *wsb = static_cast<const uint8_t *>(c->d_augws.p); // null when nothing wrote it: never read then
  const int src = colored ? kMixSrcB : augmented ? kMixSrcByCount : kMixSrcA;
  HIPCHK(c, launch_mix_apply(dmix, augmented ? static_cast<const ldt_aug *>(c->d_aug.p) : nullptr, wsa, wsb, src,
                             w.status, lut, out_img, fmt, p.n, cgeom, s));
  if (pc.mix_classes > 0)
    HIPCHK(c, launch_mix_labels(dmix, p.labels, w.status, pc.mix_soft, p.n, pc.mix_classes, s));
  return LDT_OK;
}

// The end of a staged call: its failed rows zeroed in the call's own format
// (with their labels), as every other call leaves them, and the COLOR mark.
int staged_tail(ldt_ctx *c, DevPlan &p, const DevWork &w, float *out_img, int64_t *out_lbl, OutFmt fmt,
                hipStream_t s) {
  p.ro.fmt = fmt;
  if (p.views) // several views, or a size list
    HIPCHK(c, launch_fill_failed_views(p, w, out_img, out_lbl, s));
  else
    HIPCHK(c, launch_fill_failed(p, w, out_img, out_lbl, s));
  prof_mark(c, LDT_STAGE_COLOR, s);
  return LDT_OK;
}

// The per-image status back to the host, into the slot's buffer, and the
// call's end: its ticket, the host-side statuses in `status_out`, and the
// device's merged in when the context waits for them (LDT_OPT_SYNC_STATUS).
int status_back(ldt_ctx *c, int sl, int64_t n, const int32_t *dev_status, bool plan_with_cells, const BatchPlan &B,
                int32_t *status_out, hipStream_t s, HostTimer &ht) {
  if ((size_t)n > c->h_status_cap[sl]) {
    if (c->h_status[sl]) {
      HIPCHK(c, hipEventSynchronize(c->st_ev[sl])); // its last copy has landed
      HIPCHK(c, hipHostFree(c->h_status[sl]));
    }
    c->h_status[sl] = nullptr;
    c->h_status_cap[sl] = 0;
    c->st_ticket[sl] = -1;
    if (hipHostMalloc((void **)&c->h_status[sl], 4 * (size_t)n, hipHostMallocDefault) != hipSuccess)
      return set_err(c, LDT_ERR_NOMEM, "hipHostMalloc(status) failed");
    c->h_status_cap[sl] = (size_t)n;
  }
  HIPCHK(c, hipMemcpyAsync(c->h_status[sl], dev_status, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipEventRecord(c->st_ev[sl], s));
  if (plan_with_cells) {
    // every reader of the slot's device buffer (cells and plan blob) is
    // enqueued: a later DMA into it waits for the status copy
    HIPCHK(c, hipEventRecord(c->data_free_ev[sl], s));
    c->data_used[sl] = true;
  }
  c->st_ticket[sl] = ++c->tickets;
  c->st_n[sl] = n;
  c->last_sl = sl;
  c->last_n = n;
  int rc;
  if ((rc = finish_call(c, s))) return rc;
  ht.mark(kHpStatus); // status copy enqueued
  memcpy(status_out, B.status.data(), 4 * (size_t)n);
  if (c->sync_status) {
    HIPCHK(c, hipStreamSynchronize(s));
    bool bad = false;
    for (int64_t i = 0; i < n; ++i) {
      if (status_out[i] == 0) status_out[i] = c->h_status[sl][i];
      if (status_out[i]) bad = true;
    }
    if (bad) return set_err(c, LDT_ERR_IMAGE, "one or more images failed to decode");
  } else if (B.any_bad) {
    return set_err(c, LDT_ERR_IMAGE, "one or more images failed to parse");
  }
  return LDT_OK;
}

// Core of every JPEG decode entry point.
//   data_host: cells (host); cell i = [off(i) - base, off(i+1) - base)
//   data_dev : if non-null, the cells already live in HBM at the same offsets.
template <typename OffT>
int decode_core(ldt_ctx *c, const uint8_t *data_host, const uint8_t *data_dev, const OffT *offsets,
                int64_t arr_offset, int64_t n, const uint8_t *validity, const int64_t *labels,
                int64_t label_offset, float *out_img, int64_t *out_lbl, const ldt_norm *norm,
                hipStream_t s, int32_t *status_out) {
  if (!c) return LDT_ERR_ARG;
  const PendingCall pc = take_pending(c); // first thing: whatever becomes of the call
  CallShape cs;
  int rc;
  if ((rc = check_call(c, pc, n, n <= 0 || (data_host && offsets && out_img && status_out), norm, cs,
                       labels && n > 0 ? labels + label_offset : nullptr)))
    return rc;
  if (n == 0) return LDT_OK;
  if (labels && !out_lbl) return set_err(c, LDT_ERR_ARG, "labels given without out_lbl");
  const bool boxed = pc.boxed, windowed = pc.windowed, colored = pc.colored, augmented = pc.augmented;
  const bool mixed = pc.mixed;
  const bool staged = colored || augmented || mixed; // the resize writes the workspace, a later stage the output
  const bool sized = cs.sized;
  const int views = cs.views;
  const OutFmt fmt = c->fmt;
  DeviceGuard g(c->device);
  if ((rc = order_streams(c, s))) return rc;
  HostTimer ht(c);
  const int64_t base = (int64_t)offsets[arr_offset];
  const int64_t total_bytes = (int64_t)offsets[arr_offset + n] - base;
  if (total_bytes < 0) return set_err(c, LDT_ERR_ARG, "offsets not monotonic");
  const uint8_t *cells_host = data_host + base; // cell i at cells_host + (offsets[i] - base)
  if (c->coef_dirty) {
    // an earlier call failed between the Huffman and IDCT launches
    if (c->d_pcoef.p) HIPCHK(c, hipMemsetAsync(c->d_pcoef.p, 0, c->d_pcoef.cap, s));
    c->coef_dirty = false;
  }

  // ---- pinned slot, then the cells' way to HBM, which the header walk below
  // overlaps: the pool threads copy them into the slot (a registered range is
  // DMAed from the caller's pages at once). The copy is joined after the
  // header walk and the batch goes to HBM in one DMA (enqueue_cells). ----
  if ((rc = acquire_slot(c))) return rc;
  const int sl = c->slot;
  std::shared_ptr<HostRange> reg; // registered range the H2D reads from
  CopyJoin cj;
  prof_begin(c, LDT_STAGE_H2D, s);
  if (!data_dev && total_bytes > 0) {
    if ((rc = ensure_dev(c, c->d_data[sl], (size_t)total_bytes + 16, s))) return rc;
    reg = host_acquire(cells_host, (size_t)total_bytes, c->device);
    if (reg) {
      if ((rc = enqueue_cells(c, sl, cells_host, (size_t)total_bytes, s))) return rc;
    } else {
      // room for the plan blob after the cells (plan_with_cells below)
      const size_t room = (size_t)total_bytes + 16 + std::max<size_t>((size_t)total_bytes / 8, (size_t)1 << 18);
      if ((rc = ensure_pin_slots(c, c->h_data, sl, room))) return rc;
      CopyPool &pool = copier(c);
      pool.start(c->h_data[sl].p, cells_host, (size_t)total_bytes);
      cj.p = &pool;
    }
  }
  struct RegRelease {
    std::shared_ptr<HostRange> &r;
    ~RegRelease() { host_release(r); }
  } reg_release{reg};
  ht.mark(kHpSlot);

  // ---- plan the batch from the cells' headers (ldt_plan.cpp) ----
  PlanOptions opt;
  opt.parallel = c->huff_mode != 1;
  opt.subseq_bits = c->subseq_bits;
  opt.fuse_destuff = c->fuse_destuff;
  opt.win_cap = c->win_cap;
  opt.out_h = c->out_h;
  opt.out_w = c->out_w;
  const int filter = c->filter;
  opt.filter = filter;
  BatchPlan B;
  plan_batch(data_host, offsets, arr_offset, n, validity, opt, c->huff, B, boxed ? pc.crops.data() : nullptr,
             windowed ? pc.windows.data() : nullptr, views, sized ? pc.view_sizes.data() : nullptr,
             pc.drafted ? pc.drafts.data() : nullptr);
  if (B.geom_bad) return set_err(c, LDT_ERR_ARG, "view sizes refused by the planner");
  ht.mark(kHpParse); // headers parsed, per-image plans built
  const PlanLayout L = plan_layout(B, labels != nullptr);
  const int64_t plan_bytes = L.plan_bytes;

  // Host cells copied into the pinned slot: the plan blob follows them in the
  // slot and reaches HBM in the same DMA (a separate small H2D copy would be
  // enqueued behind the stream's wait for that DMA, and the runtime may
  // perform small copies synchronously). Otherwise its own pinned buffer and
  // copy on `s`.
  const int64_t plan_off = (total_bytes + 16 + 255) & ~(int64_t)255;
  const bool plan_with_cells = cj.p != nullptr && (int64_t)c->h_data[sl].cap >= plan_off + plan_bytes;
  uint8_t *hp;
  if (plan_with_cells) {
    hp = static_cast<uint8_t *>(c->h_data[sl].p) + plan_off;
  } else {
    if ((rc = ensure_pin_slots(c, c->h_plan, sl, (size_t)plan_bytes))) return rc;
    hp = static_cast<uint8_t *>(c->h_plan[sl].p);
  }
  write_plan(B, L, norm, labels ? labels + label_offset : nullptr, hp, fmt.dtype);

  // ---- device workspace ----
  if (plan_with_cells) {
    if ((rc = ensure_dev(c, c->d_data[sl], (size_t)(plan_off + plan_bytes), s))) return rc;
  } else if ((rc = ensure_dev(c, c->d_plan, (size_t)plan_bytes, s))) {
    return rc;
  }
  // slack: a decoder finishing its last block may read a few hundred bytes
  // past an image's region
  if ((rc = ensure_dev(c, c->d_dstuf, (size_t)B.dst_total + 1024, s))) return rc;
  // packed coefficients and block records: written before they are read in
  // every batch; the progressive planes: all zero between batches (k_idct
  // clears what it reads), so they are zeroed only when allocated
  if ((rc = ensure_dev(c, c->d_coef, (size_t)B.coef_blocks * 128 + 256, s))) return rc;
  if ((rc = ensure_dev(c, c->d_brec, (size_t)B.coef_blocks * 4 + 64, s))) return rc;
  if ((rc = ensure_dev(c, c->d_bcarry, (size_t)B.coef_blocks / 16 + 64, s))) return rc;
  if (B.pcoef_blocks > 0 && (rc = ensure_dev(c, c->d_pcoef, (size_t)B.pcoef_blocks * 128 + 64, s, true))) return rc;
  if ((rc = ensure_dev(c, c->d_dcv, (size_t)B.coef_blocks * 2 + 64, s))) return rc;
  if ((rc = ensure_dev(c, c->d_planes, (size_t)B.plane_total + 64, s))) return rc;
  if ((rc = ensure_dev(c, c->d_dscnt, 16 * (size_t)(B.n_chunks + 1), s))) return rc;
  const ColorGeom &cgeom = cs.cgeom;
  const int aug_k = cs.aug_k;
  StagedEntries entries;
  ColorStage col;
  bool aug_stats[LDT_MAX_AUG_OPS] = {}; // slots in which some entry's op needs the statistics pass
  if (staged) {
    // the resized bytes of every output image, laid out as the output is
    const size_t ws_bytes = (size_t)(cgeom.base[views - 1] + n * 3 * cgeom.oh[views - 1] * cgeom.ow[views - 1]);
    if ((rc = ensure_dev(c, c->d_colws, ws_bytes + 16, s))) return rc;
    // the second workspace: the augment ops' ping-pong, or what the colour or
    // augment stage of a call with a mix leaves for the mix kernel
    if ((aug_k > 1 || (mixed && (colored || aug_k > 0))) && (rc = ensure_dev(c, c->d_augws, ws_bytes + 16, s)))
      return rc;
  }
  StagedEntries mix_entries;
  if (mixed) {
    // the float32 table (the plan's is in the call's dtype), then the records
    mix_entries.bytes = kMixLutBytes + pc.mixes.size() * sizeof(ldt_mix);
    if ((rc = ensure_dev(c, c->d_mix, mix_entries.bytes, s))) return rc;
    if ((rc = ensure_pin_slots(c, c->h_mix, sl, mix_entries.bytes))) return rc;
    uint8_t *hm = static_cast<uint8_t *>(c->h_mix[sl].p);
    build_lut(norm, reinterpret_cast<float *>(hm));
    memcpy(hm + kMixLutBytes, pc.mixes.data(), pc.mixes.size() * sizeof(ldt_mix));
    mix_entries.dev = c->d_mix.p;
    mix_entries.pin = hm;
  }
  if (augmented) {
    if ((rc = stage_entries(c, pc.augs, c->d_aug, c->h_aug, sl, s, entries))) return rc;
    if ((rc = ensure_dev(c, c->d_augstat, (size_t)kAugStatBytes * pc.augs.size(), s))) return rc;
    for (const ldt_aug &e : pc.augs)
      for (int k = 0; k < e.count; ++k)
        if (aug_needs_stats(e.op[k].code)) aug_stats[aug_k - e.count + k] = true;
  }
  if (colored) {
    if ((rc = stage_entries(c, pc.colors, c->d_color, c->h_color, sl, s, entries))) return rc;
    if ((rc = ensure_dev(c, c->d_colsum, 4 * pc.colors.size(), s))) return rc;
    for (const ldt_color &e : pc.colors) {
      col.mean = col.mean || color_has_contrast(e);
      if (e.blur_ww != 0) col.blur_max_r = std::max(col.blur_max_r, (int)e.blur_r);
    }
    if (col.blur_max_r >= 0 && !blur_geom_build(n, cgeom, col.bgeom))
      return set_err(c, LDT_ERR_ARG, "colours: the blur's grid for %lld rows does not fit an int", (long long)n);
  }
  ht.mark(kHpPlan); // plan blob written, buffers sized
  const uint8_t *dev_cells = data_dev;
  if (!data_dev) {
    if (cj.p) {
      // every chunk copied into the slot: one DMA of the batch
      CopyPool *pool = cj.p;
      cj.wait();
      if (c->host_timing) {
        c->host_us[kHpCopyWake] += std::max(0.0, pool->last_wake_us());
        c->host_us[kHpCopySpan] += pool->last_span_us();
      }
      const size_t nb = (size_t)(plan_with_cells ? plan_off + plan_bytes : total_bytes);
      if ((rc = enqueue_cells(c, sl, c->h_data[sl].p, nb, s))) return rc;
    }
    host_release(reg);
    dev_cells = static_cast<const uint8_t *>(c->d_data[sl].p);
  }
  if (!plan_with_cells) HIPCHK(c, hipMemcpyAsync(c->d_plan.p, hp, (size_t)plan_bytes, hipMemcpyHostToDevice, s));
  if (colored || augmented) HIPCHK(c, entries.h2d(s));
  if (mixed) HIPCHK(c, mix_entries.h2d(s));
  HIPCHK(c, hipEventRecord(c->slot_ev[sl], s));
  c->slot_used[sl] = true;
  prof_mark(c, LDT_STAGE_H2D, s);
  ht.mark(kHpCopy);

  uint8_t *dp = plan_with_cells ? static_cast<uint8_t *>(c->d_data[sl].p) + plan_off
                                : static_cast<uint8_t *>(c->d_plan.p);
  DevPlan p;
  p.descs = reinterpret_cast<const ImgDesc *>(dp + L.off_desc);
  p.segs = reinterpret_cast<Segment *>(dp + L.off_seg);
  p.htabs = reinterpret_cast<const HuffTab *>(dp + L.off_huff);
  p.qtabs = reinterpret_cast<const uint16_t *>(dp + L.off_quant);
  p.lut = reinterpret_cast<const float *>(dp + L.off_lut);
  p.labels = labels ? reinterpret_cast<const int64_t *>(dp + L.off_labels) : nullptr;
  p.n = (int)n;
  p.nseg = (int)B.segs.size();
  p.max_ks_h = B.max_ks_h;
  p.max_ks_v = B.max_ks_v;
  p.max_w = B.max_w;
  p.max_h = B.max_h;
  p.max_blocks = B.max_blocks;
  p.n_par = (int)B.par_img.size();
  p.par_img = reinterpret_cast<const int32_t *>(dp + L.off_par);
  p.n_serial = B.n_serial;
  p.win_bytes = B.win_bytes;
  p.warm_pct = c->warm_pct;
  p.resize_waves_pct = c->resize_waves_pct;
  p.resize_wpg = c->resize_wpg;
  // 4:2:0 sources <= 512 px: 0 the packed 16-bit staging (k_resize4<5>),
  // 1 the 32-bit staging (k_resize4<0>)
  p.resize420 = c->resize_impl == 1 ? 0 : 3;
  p.n_chunks = B.n_chunks;
  p.n_ds_img = B.n_ds_img;
  p.chunk_img = reinterpret_cast<const int32_t *>(dp + L.off_chunk);
  // diagnostic counters only on request: their atomics cost the kernels time
  p.redo = c->debug_counters ? reinterpret_cast<int32_t *>(dp + L.off_redo) : nullptr;
  if (p.n_par > 0) p.sc = sc_view(c, s);
  p.max_tabs = B.max_tabs;
  p.n_fast420 = B.n_fast420;
  p.n_draft = B.n_draft;
  p.n_prog = (int)B.prog_img.size();
  p.prog_img = reinterpret_cast<const int32_t *>(dp + L.off_pimg);
  p.pscans = reinterpret_cast<const ProgScan *>(dp + L.off_pscan);
  p.ptabs = reinterpret_cast<const ProgTab *>(dp + L.off_ptab);
  if (views > 1 || sized) {
    p.views = reinterpret_cast<const ViewDesc *>(dp + L.off_view);
    p.n_views = views;
  }
  if (sized) p.geom = &B.geom;
  c->last_off_redo = c->debug_counters ? L.off_redo : -1;
  c->last_plan_dev = dp;
  DevWork w;
  w.data = dev_cells;
  w.dstuf = static_cast<uint8_t *>(c->d_dstuf.p);
  w.coef = static_cast<int16_t *>(c->d_coef.p);
  w.brec = static_cast<uint32_t *>(c->d_brec.p);
  w.bcarry = static_cast<uint32_t *>(c->d_bcarry.p);
  w.pcoef = static_cast<int16_t *>(c->d_pcoef.p);
  w.dcv = static_cast<int16_t *>(c->d_dcv.p);
  w.planes = static_cast<uint8_t *>(c->d_planes.p);
  w.status = reinterpret_cast<int32_t *>(dp + L.off_status);
  w.ds_cnt = static_cast<int4 *>(c->d_dscnt.p);

  // a call with colours resizes as a uint8 contiguous call does, into the
  // colour workspace; the plan's table stays in the call's own dtype for the
  // colour kernels (the uint8 resize reads none)
  p.ro.fmt = staged ? OutFmt{kDtypeU8, kLayoutNCHW} : fmt;
  float *const resize_out = staged ? static_cast<float *>(c->d_colws.p) : out_img;
  // coefficient tables of sizes not seen before: one tiny launch, ahead of
  // the batch's kernels
  if (boxed || windowed || filter != kFilterBilinear || views > 1 || sized) {
    // the streaming kernel computes its own coefficients: no tables
    p.ro.oh = c->out_h;
    p.ro.ow = c->out_w;
  } else {
    std::vector<int> ws, hs;
    ws.reserve(B.descs.size());
    hs.reserve(B.descs.size());
    for (const ImgDesc &d : B.descs) {
      ws.push_back(d.width);
      hs.push_back(d.height);
    }
    if ((rc = resize_tables(c, s, ws, hs, p.ro))) return rc;
  }
  HIPCHK(c, launch_destuff(p, w, s));
  prof_mark(c, LDT_STAGE_DESTUFF, s);
  c->coef_dirty = p.n_prog > 0; // until k_idct is enqueued behind k_prog's output
  HIPCHK(c, launch_huff_parallel(p, w, s));
  HIPCHK(c, launch_huff_serial(p, w, s));
  HIPCHK(c, launch_prog(p, w, s));
  HIPCHK(c, launch_dc_scan(p, w, s));
  if (!data_dev && !plan_with_cells) {
    // the cells' last readers are enqueued: a later DMA into this slot's
    // device buffer waits for them (copy stream). With the plan blob in the
    // same buffer, its readers (k_idct, the resize, the status copy) come
    // later: the event is recorded after the status copy below.
    HIPCHK(c, hipEventRecord(c->data_free_ev[sl], s));
    c->data_used[sl] = true;
  }
  prof_mark(c, LDT_STAGE_HUFFMAN, s);
  HIPCHK(c, launch_idct(p, w, s, &c->last_idct_scaled));
  c->coef_dirty = false;
  prof_mark(c, LDT_STAGE_IDCT, s);
  if (views > 1 || sized) {
    // several views per image: k_resize_views reads the planes once per view
    // (the view table holds every view's box and window) and writes output
    // image v * n + i; no other call launches it
    HIPCHK(c, launch_resize_views(p, w, resize_out, labels ? out_lbl : nullptr, s, filter, c->view_order));
    c->last_resize_wpg = 0;
    c->last_resize_bands = 0;
    if (!staged) HIPCHK(c, launch_fill_failed_views(p, w, out_img, labels ? out_lbl : nullptr, s));
  } else {
    // k_resize4 writes the failed images itself; the streaming fallback does not
    hipError_t rerr = hipSuccess;
    int wpg = 0, bands = 0;
    // a batch with crops takes the streaming kernel's BOX variant, one with
    // windows its BOX == 2 variant (the descriptors' box is the whole image
    // when the batch has no crops); so does every batch whose filter is not
    // BILINEAR, whatever LDT_OPT_RESIZE_IMPL says (k_resize4's unsigned
    // multiply and clamp are not safe for negative weights)
    const bool r4 = !boxed && !windowed && filter == kFilterBilinear && c->resize_impl != 2 &&
                    launch_resize4_jpeg(p, w, resize_out, labels ? out_lbl : nullptr, s, &rerr, &wpg, &bands);
    c->last_resize_wpg = r4 ? wpg : 0;
    c->last_resize_bands = r4 ? bands : 0;
    if (!r4)
      rerr = launch_resize_jpeg(p, w, resize_out, labels ? out_lbl : nullptr, s, windowed ? 2 : boxed ? 1 : 0, filter);
    HIPCHK(c, rerr);
    if (!r4 && !staged) HIPCHK(c, launch_fill_failed(p, w, out_img, labels ? out_lbl : nullptr, s));
  }
  prof_mark(c, LDT_STAGE_RESIZE, s);
  if (staged) {
    // workspace -> the call's output, then the failed rows
    // with a mix the stage before it stores uint8 planes in the second workspace
    float *const stage_out = mixed ? static_cast<float *>(c->d_augws.p) : out_img;
    const OutFmt stage_fmt = mixed ? OutFmt{kDtypeU8, kLayoutNCHW} : fmt;
    if (colored && (rc = color_stage(c, col, pc.colors.size(), p, w, stage_out, stage_fmt, cgeom, s))) return rc;
    if (augmented && (rc = augment_stage(c, aug_k, aug_stats, p, w, stage_out, stage_fmt, cgeom, s, mixed))) return rc;
    if (mixed && (rc = mix_stage(c, pc, colored, augmented, p, w, out_img, fmt, cgeom, s))) return rc;
    if ((rc = staged_tail(c, p, w, out_img, labels ? out_lbl : nullptr, fmt, s))) return rc;
  }
  c->cur_ev = nullptr;

  ht.mark(kHpLaunch); // kernels launched
  return status_back(c, sl, n, w.status, plan_with_cells, B, status_out, s, ht);
}

// The frame of the four array setters: what was pending of the kind is
// dropped; a null `src` leaves none; else `validate()` (a setter's own loop
// over the entries, which sets the error) passes before they are kept and
// `flag` says so. `what`, `unit`: the kind's words in the messages.
template <typename E, typename Validate>
int set_pending(ldt_ctx *c, std::vector<E> &dst, bool &flag, const E *src, int64_t n, const char *what,
                const char *unit, Validate validate) {
  dst.clear();
  flag = false;
  if (!src) return LDT_OK;
  if (n < 0) return set_err(c, LDT_ERR_ARG, "%s: n=%lld", what, (long long)n);
  if (int rc = validate()) return rc;
  try {
    dst.assign(src, src + n);
  } catch (...) {
    return set_err(c, LDT_ERR_NOMEM, "%s: no memory for %lld %s", what, (long long)n, unit);
  }
  flag = true;
  return LDT_OK;
}

} // namespace

// ---------------------------------------------------------------------------
// C-ABI.
// ---------------------------------------------------------------------------
extern "C" {

const char *ldt_version(void) { return "ldt 0.1.0 gfx950"; }

ldt_ctx *ldt_create(int device, size_t max_batch_bytes, int max_n) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return nullptr;
  ldt_ctx *c = new (std::nothrow) ldt_ctx();
  if (!c) return nullptr;
  c->device = device;
  DeviceGuard g(device);
  for (int k = 0; k < ldt_ctx::kSlots; ++k)
    if (hipEventCreateWithFlags(&c->slot_ev[k], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->st_ev[k], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->data_free_ev[k], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->h2d_ev[k], hipEventDisableTiming) != hipSuccess) {
      delete c;
      return nullptr;
    }
  if (hipEventCreateWithFlags(&c->done_ev, hipEventDisableTiming) != hipSuccess) {
    delete c;
    return nullptr;
  }
  if (max_batch_bytes > 0) {
    for (int k = 0; k < ldt_ctx::kSlots; ++k) (void)ensure_dev(c, c->d_data[k], max_batch_bytes, nullptr);
    for (int k = 0; k < ldt_ctx::kSlots; ++k) (void)ensure_pin(c, c->h_data[k], max_batch_bytes);
  }
  (void)max_n;
  if (device < 64) {
    std::lock_guard<std::mutex> l(g_sc_m);
    ++g_sc[device].ctxs;
  }
  return c;
}

void ldt_destroy(ldt_ctx *c) {
  if (!c) return;
  DeviceGuard g(c->device);
  (void)hipDeviceSynchronize();
  DevBuf *dbs[] = {&c->d_data[0], &c->d_data[1], &c->d_plan, &c->d_dstuf, &c->d_coef, &c->d_brec, &c->d_bcarry, &c->d_pcoef, &c->d_dcv,
                    &c->d_planes, &c->d_raw, &c->d_dscnt, &c->d_resamp, &c->d_resamp_g[0], &c->d_resamp_g[1],
                    &c->d_color, &c->d_colsum, &c->d_colws, &c->d_aug, &c->d_augstat, &c->d_augws, &c->d_mix};
  for (DevBuf *b : dbs)
    if (b->p) (void)hipFree(b->p);
  for (int k = 0; k < ldt_ctx::kSlots; ++k) {
    if (c->h_data[k].p) (void)hipHostFree(c->h_data[k].p);
    if (c->h_plan[k].p) (void)hipHostFree(c->h_plan[k].p);
    if (c->h_color[k].p) (void)hipHostFree(c->h_color[k].p);
    if (c->h_aug[k].p) (void)hipHostFree(c->h_aug[k].p);
    if (c->h_mix[k].p) (void)hipHostFree(c->h_mix[k].p);
    if (c->slot_ev[k]) (void)hipEventDestroy(c->slot_ev[k]);
    if (c->st_ev[k]) (void)hipEventDestroy(c->st_ev[k]);
    if (c->data_free_ev[k]) (void)hipEventDestroy(c->data_free_ev[k]);
    if (c->h2d_ev[k]) (void)hipEventDestroy(c->h2d_ev[k]);
    if (c->h_status[k]) (void)hipHostFree(c->h_status[k]);
  }
  if (c->done_ev) (void)hipEventDestroy(c->done_ev);
  if (c->device >= 0 && c->device < 64) {
    // the device's sync cache goes with its last context
    std::lock_guard<std::mutex> l(g_sc_m);
    ScTable &t = g_sc[c->device];
    if (--t.ctxs <= 0) {
      t.ctxs = 0;
      sc_free_locked(t);
    }
  }
  delete c;
}

const char *ldt_last_error(ldt_ctx *c) { return c ? c->err.c_str() : "null context"; }

int ldt_register_host(ldt_ctx *c, const void *ptr, size_t len) {
  if (!c || !ptr || len == 0) return c ? set_err(c, LDT_ERR_ARG, "register: empty range") : LDT_ERR_ARG;
  DeviceGuard g(c->device);
  if (host_registered(ptr, len)) return LDT_OK;
  hipError_t e = hipHostRegister(const_cast<void *>(ptr), len, hipHostRegisterDefault);
  if (e != hipSuccess) { // e.g. a read-only mapping
    (void)hipGetLastError();
    e = hipHostRegister(const_cast<void *>(ptr), len, hipHostRegisterReadOnly);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return set_err(c, LDT_ERR_HIP, "hipHostRegister(%zu bytes): %s", len, hipGetErrorString(e));
  }
  auto r = std::make_shared<HostRange>();
  r->lo = (uintptr_t)ptr;
  r->hi = (uintptr_t)ptr + len;
  std::lock_guard<std::mutex> l(g_host_m);
  g_host_ranges.push_back(std::move(r));
  return LDT_OK;
}

int ldt_unregister_host(ldt_ctx *c, const void *ptr) {
  if (!c) return LDT_ERR_ARG;
  DeviceGuard g(c->device);
  uint64_t devmask;
  {
    // no new decode picks the range up once it is out of the list; wait for
    // the ones that did until they have enqueued their copies
    std::unique_lock<std::mutex> l(g_host_m);
    auto it = std::find_if(g_host_ranges.begin(), g_host_ranges.end(),
                           [&](const std::shared_ptr<HostRange> &r) { return r->lo == (uintptr_t)ptr; });
    if (it == g_host_ranges.end()) return set_err(c, LDT_ERR_ARG, "unregister: range not registered");
    std::shared_ptr<HostRange> r = *it;
    g_host_ranges.erase(it);
    g_host_cv.wait(l, [&] { return r->inflight == 0; });
    devmask = r->devmask;
  }
  // every device that copied from the range has finished doing so
  for (int d = 0; d < 64; ++d) {
    if (!((devmask >> d) & 1)) continue;
    DeviceGuard gd(d);
    HIPCHK(c, hipDeviceSynchronize());
  }
  HIPCHK(c, hipHostUnregister(const_cast<void *>(ptr)));
  return LDT_OK;
}

// The stream a context's cells go to HBM on in LDT_OPT_COPY_MODE 0 (NULL:
// the device's own copy stream). A caller that owns its streams lends one
// here, so that the DMAs do not add a fifth stream to the process's four
// hardware queues (DecodePipeline's adaptive mode, transforms.py).
int ldt_set_copy_stream(ldt_ctx *c, void *stream) {
  if (!c) return LDT_ERR_ARG;
  c->copy_stream = (hipStream_t)stream;
  return LDT_OK;
}

int ldt_set_option(ldt_ctx *c, int option, int64_t value) {
  if (!c) return LDT_ERR_ARG;
  switch (option) {
  case LDT_OPT_SYNC_STATUS:
    c->sync_status = value != 0;
    return LDT_OK;
  case LDT_OPT_HUFF_MODE:
    if (value < 0 || value > 2) return set_err(c, LDT_ERR_ARG, "huff mode %lld", (long long)value);
    c->huff_mode = (int)value;
    return LDT_OK;
  case LDT_OPT_PROFILE:
    c->profile = value != 0;
    return LDT_OK;
  case LDT_OPT_SYNC_WARM:
    if (value < 0 || value > 200) return set_err(c, LDT_ERR_ARG, "sync warm-up %lld", (long long)value);
    c->warm_pct = (int)value;
    return LDT_OK;
  case LDT_OPT_HUFF_WINDOW:
    if (value < -1 || value > kHuffLdsMax) return set_err(c, LDT_ERR_ARG, "window cap %lld", (long long)value);
    c->win_cap = value;
    return LDT_OK;
  case LDT_OPT_DEBUG_COUNTERS:
    c->debug_counters = value != 0;
    return LDT_OK;
  case LDT_OPT_SYNC_CACHE:
    if (value < 0 || value > 2) return set_err(c, LDT_ERR_ARG, "sync cache %lld", (long long)value);
    c->sync_cache = (int)value;
    return LDT_OK;
  case LDT_OPT_SYNC_CACHE_MB: {
    if (value < 0 || value > 65536) return set_err(c, LDT_ERR_ARG, "sync cache budget %lld MiB", (long long)value);
    if (c->device < 0 || c->device >= 64) return LDT_OK;
    DeviceGuard g(c->device);
    std::lock_guard<std::mutex> l(g_sc_m);
    ScTable &t = g_sc[c->device];
    if (t.budget_mb != value) { // a new table (empty) with the next decode
      sc_free_locked(t);
      t.budget_mb = value;
    }
    return LDT_OK;
  }
  case LDT_OPT_RESIZE_IMPL:
    if (value < 0 || value > 3) return set_err(c, LDT_ERR_ARG, "resize impl %lld", (long long)value);
    c->resize_impl = (int)value;
    return LDT_OK;
  case LDT_OPT_SUBSEQ_BITS:
    if (value < 64 || value > 8192 || (value & 31))
      return set_err(c, LDT_ERR_ARG, "subsequence bits %lld", (long long)value);
    c->subseq_bits = (int)value;
    return LDT_OK;
  case LDT_OPT_COPY_THREADS:
    if (value < -1 || value > 31) return set_err(c, LDT_ERR_ARG, "copy threads %lld", (long long)value);
    if ((int)value != c->copy_threads) {
      c->copy_threads = (int)value;
      c->copier.reset(); // rebuilt with the new size on the next copy
    }
    return LDT_OK;
  case LDT_OPT_HOST_TIMING:
    c->host_timing = value != 0;
    return LDT_OK;
  case LDT_OPT_RESIZE_WAVES_PCT:
    if (value < 10 || value > 1000) return set_err(c, LDT_ERR_ARG, "resize waves %lld%%", (long long)value);
    c->resize_waves_pct = (int)value;
    return LDT_OK;
  case LDT_OPT_RESIZE_WG_WAVES:
    if (value != 0 && value != 1 && value != 2 && value != 4)
      return set_err(c, LDT_ERR_ARG, "resize waves per workgroup %lld", (long long)value);
    c->resize_wpg = (int)value;
    return LDT_OK;
  case LDT_OPT_FUSED_DESTUFF:
    c->fuse_destuff = value != 0;
    return LDT_OK;
  case LDT_OPT_COPY_MODE:
    if (value < 0 || value > 1) return set_err(c, LDT_ERR_ARG, "copy mode %lld", (long long)value);
    c->copy_mode = (int)value;
    return LDT_OK;
  case LDT_OPT_COPY_BIND:
    if (value < 0 || value > 2) return set_err(c, LDT_ERR_ARG, "copy bind %lld", (long long)value);
    if ((int)value != c->copy_bind) {
      c->copy_bind = (int)value;
      c->copier.reset();
    }
    return LDT_OK;
  case LDT_OPT_VIEW_ORDER:
    if (value < 0 || value > 1) return set_err(c, LDT_ERR_ARG, "view order %lld", (long long)value);
    c->view_order = (int)value;
    return LDT_OK;
  case LDT_OPT_COPY_NT:
    if ((value != 0) != c->copy_nt) {
      c->copy_nt = value != 0;
      c->copier.reset();
    }
    return LDT_OK;
  default:
    return set_err(c, LDT_ERR_ARG, "unknown option %d", option);
  }
}

// The output size [out_h, out_w] of every later decode / resize call on the
// context. Host state only: calls already made carry their size with them.
static_assert(kMaxOut == LDT_MAX_OUT, "ldt.h and ldt_types.hpp disagree");
int ldt_set_output_size(ldt_ctx *c, int out_h, int out_w) {
  if (!c) return LDT_ERR_ARG;
  if (out_h < 1 || out_h > LDT_MAX_OUT || out_w < 1 || out_w > LDT_MAX_OUT)
    return set_err(c, LDT_ERR_ARG, "output size %dx%d outside 1..%d", out_h, out_w, LDT_MAX_OUT);
  c->out_h = out_h;
  c->out_w = out_w;
  return LDT_OK;
}

int ldt_set_crops(ldt_ctx *c, const ldt_crop *crops, int64_t n) {
  if (!c) return LDT_ERR_ARG;
  return set_pending(c, c->pending.crops, c->pending.boxed, crops, n, "crops", "rows", [] { return LDT_OK; });
}

int ldt_set_draft(ldt_ctx *c, const int32_t *scales, int64_t n) {
  if (!c) return LDT_ERR_ARG;
  return set_pending(c, c->pending.drafts, c->pending.drafted, scales, n, "draft", "rows", [&]() -> int {
    for (int64_t i = 0; i < n; ++i)
      if (scales[i] != 1 && scales[i] != 2 && scales[i] != 4 && scales[i] != 8)
        return set_err(c, LDT_ERR_ARG, "draft: row %lld has scale %d, not 1, 2, 4 or 8", (long long)i, (int)scales[i]);
    return LDT_OK;
  });
}

int ldt_set_windows(ldt_ctx *c, const ldt_window *windows, int64_t n) {
  if (!c) return LDT_ERR_ARG;
  return set_pending(c, c->pending.windows, c->pending.windowed, windows, n, "windows", "rows",
                     [] { return LDT_OK; });
}

static_assert(sizeof(ldt_color) == 32, "ldt_color is 32 bytes");
int ldt_set_colors(ldt_ctx *c, const ldt_color *colors, int64_t n) {
  if (!c) return LDT_ERR_ARG;
  return set_pending(c, c->pending.colors, c->pending.colored, colors, n, "colours", "entries", [&]() -> int {
    for (int64_t i = 0; i < n; ++i) {
      const ldt_color &e = colors[i];
      const float f[3] = {e.brightness, e.contrast, e.saturation};
      for (int k = 0; k < 3; ++k)
        if (((e.mask >> k) & 1) && !(f[k] >= 0.0f && f[k] <= 3.4028234664e38f)) // NaN fails both
          return set_err(c, LDT_ERR_ARG, "colour entry %lld: factor %d is not finite and >= 0", (long long)i, k);
      int seen = 0;
      for (int k = 0; k < 4; ++k) seen |= e.order[k] < 4 ? 1 << e.order[k] : 16;
      if (seen != 15)
        return set_err(c, LDT_ERR_ARG, "colour entry %lld: order is not a permutation of 0..3", (long long)i);
      if (e.mask > 15 || e.gray > 1 || e.hue_shift < 0 || e.hue_shift > 255 || e.solarize < -1 || e.solarize > 256)
        return set_err(c, LDT_ERR_ARG, "colour entry %lld: mask, gray, hue_shift or solarize out of range",
                       (long long)i);
      if (e.blur_r > kBlurMaxR || (e.blur_ww != 0 && !blur_pair_ok(e.blur_r, e.blur_ww)))
        return set_err(c, LDT_ERR_ARG, "colour entry %lld: blur_r %d, blur_ww %u is no pair ldt_blur_weights gives",
                       (long long)i, (int)e.blur_r, (unsigned)e.blur_ww);
    }
    return LDT_OK;
  });
}

static_assert(sizeof(ldt_aug_op) == 40 && sizeof(ldt_aug) == 192, "ldt_aug is 192 bytes");
int ldt_set_augments(ldt_ctx *c, const ldt_aug *augs, int64_t n) {
  if (!c) return LDT_ERR_ARG;
  return set_pending(c, c->pending.augs, c->pending.augmented, augs, n, "augments", "entries", [&]() -> int {
    for (int64_t i = 0; i < n; ++i) {
      const ldt_aug &e = augs[i];
      if (e.count < 0 || e.count > LDT_MAX_AUG_OPS)
        return set_err(c, LDT_ERR_ARG, "augment entry %lld: count %d is outside 0..%d", (long long)i, (int)e.count,
                       LDT_MAX_AUG_OPS);
      if (e.erase[2] != 0 && (e.erase[0] < 0 || e.erase[1] < 0 || e.erase[2] < 1 || e.erase[3] < 1))
        return set_err(c, LDT_ERR_ARG, "augment entry %lld: the erase box needs top, left >= 0 and height, width >= 1",
                       (long long)i);
      for (int k = 0; k < e.count; ++k) {
        const ldt_aug_op &o = e.op[k];
        if (o.code < 0 || o.code >= kAugOpCodes)
          return set_err(c, LDT_ERR_ARG, "augment entry %lld: op %d has code %d", (long long)i, k, (int)o.code);
        const bool enhance = o.code == LDT_AUG_BRIGHTNESS || o.code == LDT_AUG_COLOR || o.code == LDT_AUG_CONTRAST ||
                             o.code == LDT_AUG_SHARPNESS;
        if (enhance && !(o.factor >= 0.0f && o.factor <= 3.4028234664e38f)) // NaN fails both
          return set_err(c, LDT_ERR_ARG, "augment entry %lld: op %d's factor is not finite and >= 0", (long long)i, k);
        if ((o.code == LDT_AUG_POSTERIZE && (o.param < 0 || o.param > 8)) ||
            (o.code == LDT_AUG_SOLARIZE && (o.param < 0 || o.param > 256)))
          return set_err(c, LDT_ERR_ARG, "augment entry %lld: op %d's bits or threshold is out of range",
                         (long long)i, k);
      }
    }
    return LDT_OK;
  });
}

static_assert(sizeof(ldt_mix) == 40, "ldt_mix is 40 bytes");
int ldt_set_mix(ldt_ctx *c, const ldt_mix *rows, int64_t n, int32_t num_classes, float *out_soft_dev) {
  if (!c) return LDT_ERR_ARG;
  c->pending.mix_classes = 0;
  c->pending.mix_soft = nullptr;
  const int rc = set_pending(c, c->pending.mixes, c->pending.mixed, rows, n, "mix", "rows", [&]() -> int {
    if (num_classes < 0 || num_classes > (1 << 20))
      return set_err(c, LDT_ERR_ARG, "mix: num_classes %d is outside 0..%d", (int)num_classes, 1 << 20);
    if (num_classes > 0 && !out_soft_dev)
      return set_err(c, LDT_ERR_ARG, "mix: num_classes %d without a soft-label buffer", (int)num_classes);
    const auto finite = [](float v) { return v >= -3.4028234664e38f && v <= 3.4028234664e38f; }; // NaN fails both
    for (int64_t i = 0; i < n; ++i) {
      const ldt_mix &m = rows[i];
      if (m.partner < 0 || m.partner >= n)
        return set_err(c, LDT_ERR_ARG, "mix row %lld: partner %d is outside 0..%lld", (long long)i, (int)m.partner,
                       (long long)n - 1);
      if (!finite(m.w_self) || !finite(m.w_partner) || !finite(m.lw_self) || !finite(m.lw_partner))
        return set_err(c, LDT_ERR_ARG, "mix row %lld: a weight is not finite", (long long)i);
      if (m.box[2] != 0 && (m.box[0] < 0 || m.box[1] < 0 || m.box[2] < 1 || m.box[3] < 1))
        return set_err(c, LDT_ERR_ARG, "mix row %lld: the box needs top, left >= 0 and height, width >= 1",
                       (long long)i);
    }
    return LDT_OK;
  });
  if (rc == LDT_OK && c->pending.mixed) {
    c->pending.mix_classes = num_classes;
    c->pending.mix_soft = num_classes > 0 ? out_soft_dev : nullptr;
  }
  return rc;
}

int ldt_blur_weights(float radius, int32_t *r, uint32_t *ww) {
  if (!r || !ww) return LDT_ERR_ARG;
  return blur_weights(radius, *r, *ww) ? LDT_OK : LDT_ERR_ARG;
}

static_assert(kMaxViews == LDT_MAX_VIEWS, "ldt.h and ldt_types.hpp disagree");
int ldt_set_view_sizes(ldt_ctx *c, const int32_t *hw, int views) {
  if (!c) return LDT_ERR_ARG;
  if (!hw || views < 1 || views > LDT_MAX_VIEWS)
    return set_err(c, LDT_ERR_ARG, "view sizes: %d views outside 1..%d, or no sizes", views, LDT_MAX_VIEWS);
  for (int v = 0; v < 2 * views; ++v)
    if (hw[v] < 1 || hw[v] > LDT_MAX_OUT)
      return set_err(c, LDT_ERR_ARG, "view %d: size %dx%d outside 1..%d", v / 2, hw[v & ~1], hw[v | 1], LDT_MAX_OUT);
  try {
    c->pending.view_sizes.assign(hw, hw + 2 * views);
  } catch (...) {
    return set_err(c, LDT_ERR_NOMEM, "view sizes: no memory");
  }
  return LDT_OK;
}

int ldt_set_views(ldt_ctx *c, int views) {
  if (!c) return LDT_ERR_ARG;
  if (views < 1 || views > LDT_MAX_VIEWS)
    return set_err(c, LDT_ERR_ARG, "views %d outside 1..%d", views, LDT_MAX_VIEWS);
  c->pending.views = views;
  return LDT_OK;
}

static_assert(kFilterBilinear == LDT_FILTER_BILINEAR && kFilterBicubic == LDT_FILTER_BICUBIC,
              "ldt.h and ldt_types.hpp disagree");
int ldt_set_filter(ldt_ctx *c, int filter) {
  if (!c) return LDT_ERR_ARG;
  if (filter != LDT_FILTER_BILINEAR && filter != LDT_FILTER_BICUBIC)
    return set_err(c, LDT_ERR_ARG, "filter %d is neither LDT_FILTER_BILINEAR nor LDT_FILTER_BICUBIC", filter);
  c->filter = filter;
  return LDT_OK;
}

int ldt_get_filter(ldt_ctx *c, int *filter) {
  if (!c) return LDT_ERR_ARG;
  if (filter) *filter = c->filter;
  return LDT_OK;
}

static_assert(kDtypeF32 == LDT_DTYPE_F32 && kDtypeF16 == LDT_DTYPE_F16 && kDtypeBF16 == LDT_DTYPE_BF16 &&
                  kDtypeU8 == LDT_DTYPE_U8 && kLayoutNCHW == LDT_LAYOUT_NCHW && kLayoutNHWC == LDT_LAYOUT_NHWC,
              "ldt.h and ldt_types.hpp disagree");
int ldt_set_output_format(ldt_ctx *c, int dtype, int layout) {
  if (!c) return LDT_ERR_ARG;
  if (dtype < LDT_DTYPE_F32 || dtype > LDT_DTYPE_U8)
    return set_err(c, LDT_ERR_ARG, "dtype %d is none of LDT_DTYPE_F32, _F16, _BF16, _U8", dtype);
  if (layout != LDT_LAYOUT_NCHW && layout != LDT_LAYOUT_NHWC)
    return set_err(c, LDT_ERR_ARG, "layout %d is neither LDT_LAYOUT_NCHW nor LDT_LAYOUT_NHWC", layout);
  c->fmt.dtype = dtype;
  c->fmt.layout = layout;
  return LDT_OK;
}

int ldt_get_output_format(ldt_ctx *c, int *dtype, int *layout) {
  if (!c) return LDT_ERR_ARG;
  if (dtype) *dtype = c->fmt.dtype;
  if (layout) *layout = c->fmt.layout;
  return LDT_OK;
}

int ldt_get_output_size(ldt_ctx *c, int *out_h, int *out_w) {
  if (!c) return LDT_ERR_ARG;
  if (out_h) *out_h = c->out_h;
  if (out_w) *out_w = c->out_w;
  return LDT_OK;
}

int ldt_decode_batch(ldt_ctx *c, const uint8_t *data, const int32_t *offsets, int64_t arr_offset,
                     int64_t n, const uint8_t *validity, const int64_t *labels,
                     int64_t label_offset, float *out_img_dev, int64_t *out_lbl_dev,
                     const ldt_norm *norm, void *stream, int32_t *per_image_status) {
  return decode_core<int32_t>(c, data, nullptr, offsets, arr_offset, n, validity, labels,
                              label_offset, out_img_dev, out_lbl_dev, norm, (hipStream_t)stream,
                              per_image_status);
}

int ldt_decode_batch_large(ldt_ctx *c, const uint8_t *data, const int64_t *offsets,
                           int64_t arr_offset, int64_t n, const uint8_t *validity,
                           const int64_t *labels, int64_t label_offset, float *out_img_dev,
                           int64_t *out_lbl_dev, const ldt_norm *norm, void *stream,
                           int32_t *per_image_status) {
  return decode_core<int64_t>(c, data, nullptr, offsets, arr_offset, n, validity, labels,
                              label_offset, out_img_dev, out_lbl_dev, norm, (hipStream_t)stream,
                              per_image_status);
}

int ldt_decode_batch_resident(ldt_ctx *c, const uint8_t *data_host, const uint8_t *data_dev,
                              const int64_t *offsets, int64_t n, const int64_t *labels,
                              float *out_img_dev, int64_t *out_lbl_dev, const ldt_norm *norm,
                              void *stream, int32_t *per_image_status) {
  if (!data_dev || (c && n > 0 && offsets && offsets[0] != 0)) {
    if (c) take_pending(c); // a refused call consumes its pending options too
    return set_err(c, LDT_ERR_ARG, !data_dev ? "data_dev is null" : "resident offsets must start at 0");
  }
  return decode_core<int64_t>(c, data_host, data_dev, offsets, 0, n, nullptr, labels, 0,
                              out_img_dev, out_lbl_dev, norm, (hipStream_t)stream,
                              per_image_status);
}

int ldt_host_info(ldt_ctx *c, char *buf, size_t len) {
  if (!c || !buf || len == 0) return LDT_ERR_ARG;
  DeviceGuard g(c->device);
  (void)copier(c); // placement of the pool the next copy uses
  const CopyPlacement &P = c->placement;
  std::string cpus;
  for (size_t i = 0; i < P.cpus.size(); ++i) cpus += (i ? "," : "") + std::to_string(P.cpus[i]);
  const int w = snprintf(buf, len,
                         "{\"copy_threads\": %d, \"copy_cpus\": [%s], \"gpu_numa\": %d, \"quota_cpus\": %.2f, "
                         "\"local_rank\": %d, \"local_world\": %d, \"l3_domains\": %d, \"candidate_cores\": %d, "
                         "\"copy_bind\": %d, \"copy_nt\": %d, \"copy_mode\": %d, \"local_cpulist\": \"%s\"}",
                         (int)P.cpus.size(), cpus.c_str(), P.gpu_numa, P.quota_cpus, P.local_rank, P.local_world,
                         P.l3_domains, P.candidates, c->copy_bind, c->copy_nt ? 1 : 0, c->copy_mode,
                         P.local_cpulist.c_str());
  return w >= 0 && (size_t)w < len ? LDT_OK : set_err(c, LDT_ERR_ARG, "host info: buffer of %zu bytes too small", len);
}

int ldt_host_times(ldt_ctx *c, double *us_out, int64_t *calls_out, int reset) {
  if (!c) return LDT_ERR_ARG;
  for (int k = 0; k < kHpCount; ++k) {
    if (us_out) us_out[k] = c->host_us[k];
    if (reset) c->host_us[k] = 0;
  }
  if (calls_out) *calls_out = c->host_calls;
  if (reset) c->host_calls = 0;
  return LDT_OK;
}

int ldt_stage_times(ldt_ctx *c, double *ms_out, int64_t *count_out, int reset) {
  if (!c) return LDT_ERR_ARG;
  DeviceGuard g(c->device);
  for (auto &es : c->ev_pending) {
    HIPCHK(c, hipEventSynchronize(es.ev[es.last_stage]));
    for (int k = es.first_stage; k < es.last_stage; ++k) {
      float ms = 0.f;
      HIPCHK(c, hipEventElapsedTime(&ms, es.ev[k], es.ev[k + 1]));
      c->stage_ms[k] += ms;
      c->stage_cnt[k] += 1;
    }
    c->ev_free.push_back(es);
  }
  c->ev_pending.clear();
  for (int k = 0; k < LDT_NUM_STAGES; ++k) {
    if (ms_out) ms_out[k] = c->stage_ms[k];
    if (count_out) count_out[k] = c->stage_cnt[k];
    if (reset) {
      c->stage_ms[k] = 0;
      c->stage_cnt[k] = 0;
    }
  }
  return LDT_OK;
}

namespace {
int merge_status(ldt_ctx *c, int sl, int32_t *st, int64_t n) {
  if (n > c->st_n[sl]) return set_err(c, LDT_ERR_ARG, "n exceeds that batch");
  bool bad = false;
  for (int64_t i = 0; i < n; ++i) {
    if (st[i] == 0) st[i] = c->h_status[sl][i];
    if (st[i]) bad = true;
  }
  return bad ? set_err(c, LDT_ERR_IMAGE, "one or more images failed to decode") : LDT_OK;
}
} // namespace

int ldt_fetch_status(ldt_ctx *c, void *stream, int32_t *st, int64_t n) {
  if (!c || !st) return LDT_ERR_ARG;
  DeviceGuard g(c->device);
  HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
  if (c->tickets == 0) return n == 0 ? LDT_OK : set_err(c, LDT_ERR_ARG, "no decode yet");
  return merge_status(c, c->last_sl, st, n);
}

int64_t ldt_last_ticket(ldt_ctx *c) { return c ? c->tickets : -1; }

int ldt_fetch_status_ticket(ldt_ctx *c, int64_t ticket, int32_t *st, int64_t n) {
  if (!c || !st) return LDT_ERR_ARG;
  DeviceGuard g(c->device);
  for (int k = 0; k < ldt_ctx::kSlots; ++k)
    if (c->st_ticket[k] == ticket && ticket > 0) {
      HIPCHK(c, hipEventSynchronize(c->st_ev[k]));
      return merge_status(c, k, st, n);
    }
  return set_err(c, LDT_ERR_ARG, "status of call %lld is no longer held (last %lld)", (long long)ticket,
                 (long long)c->tickets);
}

int ldt_resize_raw(ldt_ctx *c, const uint8_t *hwc, int hwc_is_device, int64_t n, int h, int w,
                   int64_t cell_stride, float *out_img_dev, const ldt_norm *norm, void *stream) {
  if (!c) return LDT_ERR_ARG;
  const PendingCall pc = take_pending(c); // first thing, as decode_core does
  const std::vector<ldt_crop> &crops = pc.crops;
  const std::vector<ldt_window> &windows = pc.windows;
  const bool boxed = pc.boxed, windowed = pc.windowed;
  if (pc.views != 1 || !pc.view_sizes.empty())
    return set_err(c, LDT_ERR_ARG, "raw resize: views are pending (ldt_set_views); a raw source has no decode to share");
  if (pc.colored)
    return set_err(c, LDT_ERR_ARG, "raw resize: colours are pending (ldt_set_colors); the photometric stage serves decode calls only");
  if (pc.augmented)
    return set_err(c, LDT_ERR_ARG, "raw resize: augments are pending (ldt_set_augments); the auto-augment stage serves decode calls only");
  if (pc.mixed)
    return set_err(c, LDT_ERR_ARG, "raw resize: a mix is pending (ldt_set_mix); the mix stage serves decode calls only");
  if (pc.drafted)
    return set_err(c, LDT_ERR_ARG, "raw resize: a draft is pending (ldt_set_draft); a raw source has no IDCT to scale");
  const int filter = c->filter;
  const OutFmt fmt = c->fmt;
  if (n < 0 || h <= 0 || w <= 0 || h > LDT_MAX_DIM || w > LDT_MAX_DIM || !out_img_dev ||
      (n > 0 && !hwc) || cell_stride < (int64_t)h * w * 3)
    return set_err(c, LDT_ERR_ARG, "bad raw resize arguments");
  if (fmt.dtype == kDtypeU8 && norm)
    return set_err(c, LDT_ERR_ARG, "a uint8 output (LDT_DTYPE_U8) is the resized byte itself: Normalize cannot apply");
  int box_w = 1, box_h = 1;
  // windowed: the most taps of any row's (source -> res)
  int win_ks_h = resample_ksize_host(1, 1, filter), win_ks_v = win_ks_h;
  if (boxed && (int64_t)crops.size() != n)
    return set_err(c, LDT_ERR_ARG, "crops for %lld rows, the batch has %lld", (long long)crops.size(), (long long)n);
  if (windowed && (int64_t)windows.size() != n)
    return set_err(c, LDT_ERR_ARG, "windows for %lld rows, the batch has %lld", (long long)windows.size(),
                   (long long)n);
  if (boxed || windowed) {
    // every window inside its res, every box inside the cell, and the source
    // (box or cell) within the tap limit against res (the output size without
    // windows)
    for (int64_t i = 0; i < n; ++i) {
      const ldt_crop b = boxed ? crops[(size_t)i] : ldt_crop{0, 0, h, w, 0};
      const ldt_window v = windowed ? windows[(size_t)i] : ldt_window{c->out_h, c->out_w, 0, 0};
      if (windowed && check_window(v, c->out_h, c->out_w) != LDT_IMG_OK)
        return set_err(c, LDT_ERR_ARG, "raw resize: window (res %dx%d, top %d, left %d) of row %lld for output %dx%d",
                       v.res_h, v.res_w, v.top, v.left, (long long)i, c->out_h, c->out_w);
      if (check_crop(b, w, h, v.res_h, v.res_w, filter) != LDT_IMG_OK)
        return set_err(c, LDT_ERR_ARG, "raw resize: crop (%d, %d, %d, %d, flip %d) of row %lld on %dx%d -> %dx%d",
                       b.top, b.left, b.height, b.width, b.flip, (long long)i, h, w, v.res_h, v.res_w);
      box_w = std::max(box_w, b.width);
      box_h = std::max(box_h, b.height);
      win_ks_h = std::max(win_ks_h, resample_ksize_host(b.width, v.res_w, filter));
      win_ks_v = std::max(win_ks_v, resample_ksize_host(b.height, v.res_h, filter));
    }
  } else if (resample_reduce(w, c->out_w, filter) > kMaxReduce || resample_reduce(h, c->out_h, filter) > kMaxReduce) {
    // the streaming kernel's tap limit (LDT_IMG_TOO_LARGE for a JPEG row)
    return set_err(c, LDT_ERR_ARG, "raw resize %dx%d -> %dx%d reduces by more than %d (support %d)", h, w, c->out_h,
                   c->out_w, kMaxReduce, filter_support(filter));
  }
  if (n == 0) return LDT_OK;
  DeviceGuard g(c->device);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = order_streams(c, s))) return rc;
  if ((rc = acquire_slot(c))) return rc;
  const int sl = c->slot;
  // the LUT, then the crops, then the windows
  const size_t lut_bytes = 3 * 256 * 4, crop_bytes = boxed ? sizeof(ldt_crop) * (size_t)n : 0,
               aux_bytes = lut_bytes + crop_bytes + (windowed ? sizeof(ldt_window) * (size_t)n : 0);
  if ((rc = ensure_pin(c, c->h_plan[sl], aux_bytes))) return rc;
  float *hl = static_cast<float *>(c->h_plan[sl].p);
  // the table in the form the call's dtype needs: 16-bit entries in the first half
  if (fmt.dtype == kDtypeF16 || fmt.dtype == kDtypeBF16) {
    build_lut16(norm, fmt.dtype, reinterpret_cast<uint16_t *>(hl));
    memset(reinterpret_cast<uint8_t *>(hl) + 768 * 2, 0, 768 * 2);
  } else {
    build_lut(norm, hl);
  }
  if (boxed) memcpy(static_cast<uint8_t *>(c->h_plan[sl].p) + lut_bytes, crops.data(), crop_bytes);
  if (windowed)
    memcpy(static_cast<uint8_t *>(c->h_plan[sl].p) + lut_bytes + crop_bytes, windows.data(),
           sizeof(ldt_window) * (size_t)n);
  if ((rc = ensure_dev(c, c->d_plan, aux_bytes, s))) return rc;
  const uint8_t *src = hwc;
  if (!hwc_is_device) {
    const size_t bytes = (size_t)(cell_stride * (n - 1) + (int64_t)h * w * 3);
    if ((rc = ensure_pin(c, c->h_data[sl], bytes))) return rc;
    if ((rc = ensure_dev(c, c->d_raw, bytes, s))) return rc;
    pinned_copy(c, c->h_data[sl].p, hwc, bytes);
    HIPCHK(c, hipMemcpyAsync(c->d_raw.p, c->h_data[sl].p, bytes, hipMemcpyHostToDevice, s));
    src = static_cast<const uint8_t *>(c->d_raw.p);
  }
  HIPCHK(c, hipMemcpyAsync(c->d_plan.p, hl, aux_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipEventRecord(c->slot_ev[sl], s));
  c->slot_used[sl] = true;
  ResizeOut ro;
  ro.fmt = fmt;
  if (boxed || windowed || filter != kFilterBilinear) {
    ro.oh = c->out_h;
    ro.ow = c->out_w;
  } else if ((rc = resize_tables(c, s, std::vector<int>{w}, std::vector<int>{h}, ro))) {
    return rc;
  }
  prof_begin(c, LDT_STAGE_RESIZE, s);
  {
    hipError_t rerr = hipSuccess;
    bool band = false; // k_resize4 took the call (two waves per workgroup for raw sources)
    const uint8_t *aux = static_cast<const uint8_t *>(c->d_plan.p) + lut_bytes;
    if (boxed || windowed)
      rerr = launch_resize_raw(src, cell_stride, (int)n, h, w, static_cast<const float *>(c->d_plan.p), ro.oh,
                               ro.ow, out_img_dev, s, boxed ? reinterpret_cast<const ldt_crop *>(aux) : nullptr,
                               boxed ? box_w : w, boxed ? box_h : h,
                               windowed ? reinterpret_cast<const ldt_window *>(aux + crop_bytes) : nullptr, win_ks_h,
                               win_ks_v, filter, fmt);
    else if (filter == kFilterBilinear && c->resize_impl != 2 &&
             launch_resize4_raw(src, cell_stride, (int)n, h, w, static_cast<const float *>(c->d_plan.p), ro,
                                out_img_dev, s, &rerr))
      band = true;
    else
      rerr = launch_resize_raw(src, cell_stride, (int)n, h, w, static_cast<const float *>(c->d_plan.p), ro.oh,
                               ro.ow, out_img_dev, s, nullptr, 0, 0, nullptr, 0, 0, filter, fmt);
    c->last_resize_wpg = band ? 2 : 0;
    HIPCHK(c, rerr);
  }
  prof_mark(c, LDT_STAGE_RESIZE, s);
  c->cur_ev = nullptr;
  if ((rc = finish_call(c, s))) return rc;
  if (c->sync_status) HIPCHK(c, hipStreamSynchronize(s));
  return LDT_OK;
}

int ldt_shard_ranges(ldt_ctx *c, int64_t num_rows, int64_t batch_size, int rank, int world_size,
                     int64_t *out_ranges_dev, int64_t capacity, int64_t *out_count_dev,
                     void *stream) {
  if (!c) return LDT_ERR_ARG;
  if (num_rows < 0 || batch_size <= 0 || world_size <= 0 || rank < 0 || rank >= world_size ||
      !out_count_dev || (capacity > 0 && !out_ranges_dev))
    return set_err(c, LDT_ERR_ARG, "bad shard_ranges arguments");
  DeviceGuard g(c->device);
  HIPCHK(c, launch_shard_ranges(num_rows, batch_size, rank, world_size, out_ranges_dev, capacity,
                                out_count_dev, (hipStream_t)stream));
  return LDT_OK;
}

int ldt_shard_fragments(ldt_ctx *c, const int64_t *fragment_rows_dev, int nfrag,
                        int64_t batch_size, int rank, int world_size, int64_t pad_to,
                        int64_t *out_dev, int64_t capacity, int64_t *out_count_dev,
                        int64_t *out_local_count_dev, void *stream) {
  if (!c) return LDT_ERR_ARG;
  if (nfrag < 0 || batch_size <= 0 || world_size <= 0 || rank < 0 || rank >= world_size ||
      !out_count_dev || !out_local_count_dev || (nfrag > 0 && !fragment_rows_dev) ||
      (capacity > 0 && !out_dev))
    return set_err(c, LDT_ERR_ARG, "bad shard_fragments arguments");
  DeviceGuard g(c->device);
  HIPCHK(c, launch_shard_fragments(fragment_rows_dev, nfrag, batch_size, rank, world_size, pad_to,
                                   out_dev, capacity, out_count_dev, out_local_count_dev,
                                   (hipStream_t)stream));
  return LDT_OK;
}

// torch.utils.data.DistributedSampler.__iter__ (distributed.py:107-141) on
// device: randperm (n < 2^32/20, torch's MT19937 Fisher-Yates branch), pad by
// wrapping or truncate (drop_last), stride by rank. num_samples as :94-103.
int ldt_distributed_indices(ldt_ctx *c, int64_t dataset_len, int num_replicas, int rank,
                            int shuffle, uint64_t seed, int drop_last, int64_t *out_dev,
                            int64_t capacity, int64_t *num_samples_out, void *stream) {
  if (!c) return LDT_ERR_ARG;
  if (dataset_len < 0 || num_replicas <= 0 || rank < 0 || rank >= num_replicas ||
      (capacity > 0 && !out_dev))
    return set_err(c, LDT_ERR_ARG, "bad distributed_indices arguments");
  if (dataset_len >= (int64_t)(UINT32_MAX / 20))
    return set_err(c, LDT_ERR_ARG,
                   "dataset_len %lld >= 2^32/20: torch.randperm switches to 64-bit draws",
                   (long long)dataset_len);
  const int64_t n = dataset_len, W = num_replicas;
  int64_t num_samples;
  if (drop_last && n % W != 0) {
    // math.ceil((n - W) / W) with true division (n - W may be negative)
    const int64_t a = n - W;
    num_samples = a >= 0 ? (a + W - 1) / W : -((-a) / W);
  } else {
    num_samples = (n + W - 1) / W;
  }
  if (num_samples < 0) num_samples = 0;
  if (num_samples_out) *num_samples_out = num_samples;
  if (num_samples == 0) return LDT_OK;
  if (capacity < num_samples)
    return set_err(c, LDT_ERR_ARG, "capacity %lld < num_samples %lld", (long long)capacity,
                   (long long)num_samples);
  DeviceGuard g(c->device);
  hipStream_t s = (hipStream_t)stream;
  if (shuffle) {
    int rc;
    if ((rc = ensure_dev(c, c->d_perm, (size_t)n * 4 * 3 + 64, s))) return rc;
    int32_t *base = static_cast<int32_t *>(c->d_perm.p);
    HIPCHK(c, launch_dist_shuffled((uint32_t)(seed & 0xffffffffu), n, rank, num_replicas,
                                   num_samples, base, base + n, base + 2 * n, out_dev, s));
  } else {
    HIPCHK(c, launch_dist_select(nullptr, n, rank, num_replicas, num_samples, out_dev, s));
  }
  return LDT_OK;
}

// The device's sync cache: statistics, clear and the corruption hook (ldt.h).
// All three order behind every stream of the device's contexts by waiting
// for the device.
int ldt_sync_cache_stats(ldt_ctx *c, int64_t *out8) {
  if (!c || !out8) return c ? set_err(c, LDT_ERR_ARG, "sync cache stats: null output") : LDT_ERR_ARG;
  for (int i = 0; i < kScStats; ++i) out8[i] = 0;
  if (c->device < 0 || c->device >= 64) return LDT_OK;
  DeviceGuard g(c->device);
  std::lock_guard<std::mutex> l(g_sc_m);
  const ScTable &t = g_sc[c->device];
  if (!t.p) return LDT_OK;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(out8, t.p, kScStats * sizeof(int64_t), hipMemcpyDeviceToHost));
  out8[6] = sc_entries(t.sets);
  out8[7] = sc_table_bytes(t.sets);
  return LDT_OK;
}

int ldt_sync_cache_clear(ldt_ctx *c) {
  if (!c) return LDT_ERR_ARG;
  if (c->device < 0 || c->device >= 64) return LDT_OK;
  DeviceGuard g(c->device);
  std::lock_guard<std::mutex> l(g_sc_m);
  ScTable &t = g_sc[c->device];
  t.failed = false;
  if (!t.p) return LDT_OK;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemset(t.p, 0, (size_t)sc_off_payloads(t.sets))); // statistics and headers
  HIPCHK(c, hipDeviceSynchronize());
  return LDT_OK;
}

// Host-side on purpose: the payloads come back, are changed within the value
// ranges a payload can hold, and go out again with plain copies, so the hook
// itself can reach no memory but the table's.
int ldt_sync_cache_corrupt(ldt_ctx *c, int mode) {
  if (!c) return LDT_ERR_ARG;
  if (mode < 1 || mode > 4) return set_err(c, LDT_ERR_ARG, "sync cache corrupt mode %d", mode);
  if (c->device < 0 || c->device >= 64) return 0;
  DeviceGuard g(c->device);
  std::lock_guard<std::mutex> l(g_sc_m);
  const ScTable &t = g_sc[c->device];
  if (!t.p) return 0;
  HIPCHK(c, hipDeviceSynchronize());
  const int64_t ne = sc_entries(t.sets);
  std::vector<ScHeader> hdr((size_t)ne);
  uint8_t *base = static_cast<uint8_t *>(t.p);
  HIPCHK(c, hipMemcpy(hdr.data(), base + sc_off_headers(), (size_t)ne * sizeof(ScHeader), hipMemcpyDeviceToHost));
  std::vector<int64_t> ready;
  for (int64_t e = 0; e < ne; ++e)
    if (sc_meta_state(hdr[(size_t)e].meta) == kScReady) ready.push_back(e);
  // entries of one geometry next to each other: mode 1 then swaps within it
  std::sort(ready.begin(), ready.end(), [&](int64_t a, int64_t b) {
    const uint64_t ma = hdr[(size_t)a].meta, mb = hdr[(size_t)b].meta;
    return ma != mb ? ma < mb : a < b;
  });
  const size_t n = ready.size();
  std::vector<ScSlot> pay(n * kScSlots);
  uint8_t *pbase = base + sc_off_payloads(t.sets);
  for (size_t i = 0; i < n; ++i)
    HIPCHK(c, hipMemcpy(&pay[i * kScSlots], pbase + ready[i] * kScPayloadBytes, (size_t)kScPayloadBytes,
                        hipMemcpyDeviceToHost));
  std::vector<ScSlot> out(pay);
  int changed = 0;
  for (size_t i = 0; i < n; ++i) {
    ScSlot *o = &out[i * kScSlots];
    const uint32_t geom = (uint32_t)hdr[(size_t)ready[i]].meta;
    const int S = (int)(geom & 0xFFFu) << 5, slots = (int)((geom >> 12) & 0x3FFu) + 1;
    bool did = false;
    if (mode == 1) {
      if (n >= 2) {
        memcpy(o, &pay[((i + 1) % n) * kScSlots], (size_t)kScPayloadBytes);
        did = true;
      }
    } else if (mode == 2) {
      for (int q = 0; q < slots; ++q) o[q].ex_p += 1;
      did = true;
    } else if (mode == 3) {
      // slot q + 1 with an exit at or past 2 S is not its segment's first
      for (int q = 0; q + 1 < slots && !did; ++q)
        if (o[q + 1].ex_p >= 2 * S && (o[q].bk_n >> 16) >= 1 && (o[q + 1].bk_n >> 16) < 0xFFFFu) {
          o[q].bk_n -= 1u << 16;
          o[q + 1].bk_n += 1u << 16;
          did = true;
        }
    } else {
      o[0].ex_p = 0x7FFFFFF0;  // past every segment
      o[0].bk_n = 0xFFFF00FFu; // more blocks than a slot can start, k = 255
      did = true;
    }
    if (did) {
      HIPCHK(c, hipMemcpy(pbase + ready[i] * kScPayloadBytes, o, (size_t)kScPayloadBytes, hipMemcpyHostToDevice));
      ++changed;
    }
  }
  HIPCHK(c, hipDeviceSynchronize());
  return changed;
}

// Debug hook (LDT_OPT_DEBUG_COUNTERS = 1): the parallel Huffman decoder's
// counters of the last batch, 16 int32 summed over its k_huff_image
// workgroups (ldt_huffman.hip): [0] unused, [1] workgroups (images), [2]
// convergence rounds (sum), [3] rounds (max), [4] memo adoptions, [5]
// write-pass symbols (sum over lanes), [6] write-pass symbols of each wave's
// slowest lane (sum), [7] unused, [8] setup, [9] phase 1, [10] rounds, [11]
// block-count scan, [12] write pass + DC scan (10 ns s_memrealtime ticks),
// [13] needy slots and [14] waves they ran on (summed over rounds), [15]
// unused. Without the option the kernels get no counter pointer and this
// returns LDT_ERR_ARG.
int ldt_debug_counters(ldt_ctx *c, int32_t *out16, void *stream) {
  if (!c || !out16) return LDT_ERR_ARG;
  DeviceGuard g(c->device);
  if (c->last_off_redo < 0)
    return set_err(c, LDT_ERR_ARG, "no batch decoded with LDT_OPT_DEBUG_COUNTERS = 1 yet");
  HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
  HIPCHK(c, hipMemcpy(out16, c->last_plan_dev + c->last_off_redo, 64,
                      hipMemcpyDeviceToHost));
  return LDT_OK;
}

// Test hook (not part of ldt.h's stable surface): which resize kernel the last
// batch took: k_resize4's waves per workgroup (1, 2 or 4; 2 for a raw source),
// 0 for the streaming kernel, -1 before any batch.
int ldt_debug_last_resize(ldt_ctx *c) { return c ? c->last_resize_wpg : LDT_ERR_ARG; }

// Test hook (not part of ldt.h's stable surface): the bands per image of the
// last JPEG batch's k_resize4 launch (what the queried occupancy and
// LDT_OPT_RESIZE_WAVES_PCT came to), 0 for the streaming kernel.
int ldt_debug_last_resize_bands(ldt_ctx *c) { return c ? c->last_resize_bands : LDT_ERR_ARG; }

// Test hook (not part of ldt.h's stable surface): which IDCT kernel the last
// JPEG batch launched: 1 k_idct_scaled (a good row was drafted below scale 1),
// 0 k_idct, -1 before any batch.
int ldt_debug_last_idct(ldt_ctx *c) { return c ? c->last_idct_scaled : LDT_ERR_ARG; }

// Test hook (not part of ldt.h's stable surface): how many k_fill_resample
// launches the context's coefficient cache has made (a batch whose sizes are
// all cached makes none).
int64_t ldt_debug_resample_fills(ldt_ctx *c) { return c ? c->resamp_fills : -1; }

// Test hook (not part of ldt.h's stable surface): Pillow resample coefficient
// tables computed on the device, for parity tests against the oracle.
int ldt_debug_resample_coeffs(ldt_ctx *c, int in_size, int out_size, int32_t *bounds_dev,
                              int32_t *kk_dev, void *stream) {
  if (!c) return LDT_ERR_ARG;
  DeviceGuard g(c->device);
  HIPCHK(c, launch_resample_coeffs(in_size, out_size, resample_ksize_host(in_size, out_size),
                                   bounds_dev, kk_dev, (hipStream_t)stream));
  return LDT_OK;
}

} // extern "C"
