// Host side of libldgpu: the C ABI of include/ldgpu.h (unity-built into ldgpu.hip).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <thread>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

using namespace ldg;

struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
};

}  // namespace

// comb-ntsc's defaults (comb-ntsc.cxx:15-75,1074-1091)
static inline comb::CombOpt comb_defaults() {
  comb::CombOpt c;
  c.firstline = comb::FIRST_LINE;
  c.nrows = comb::OUT_H;
  c.out_rows = comb::OUT_H;
  c.adaptive2d = 1;
  c.bw = 0;
  c.colorlpf = 1;
  c.lpq = 0;
  c.debug_row = -1;
  c.black_ire = 7.5;
  c.bright_m = 236.0 * 256 / 100;
  c.nr_y = 1.0 * comb::IRESCALE;
  c.wide = 0;
  c.of = 0;
  c.nr_c = 0.0;
  return c;
}
// whether o is comb-ntsc's defaults (the comb then runs the kernels with them folded)
static inline bool comb_is_default(const comb::CombOpt& o) {
  const comb::CombOpt d = comb_defaults();
  return o.firstline == d.firstline && o.nrows == d.nrows && o.out_rows == d.out_rows &&
         o.adaptive2d == d.adaptive2d && o.bw == d.bw && o.colorlpf == d.colorlpf && o.lpq == d.lpq &&
         o.debug_row == d.debug_row && o.black_ire == d.black_ire && o.bright_m == d.bright_m &&
         o.nr_y == d.nr_y && o.nr_c == d.nr_c && o.wide == d.wide;
}

struct CapStream;                 // stream.inc: a capture streamed from its file through an HBM ring
struct ldg_efm_state;             // efm.inc: the EFM run-length extraction's options and buffers
struct ldg_efmdec_state;          // efmdec.inc: the EFM decode's table, carried stream and buffers
struct ldg_efmsec_state;          // efmsec.inc: the EFM data sectors' tables, carried bytes and buffers
struct ldg_lines_state;           // lines.inc: the NTSC line services' buffers
struct ldg_flac_state;            // flac.inc: an open FLAC-compressed capture, its index and staging

struct ldg_ctx {
  int device = 0;
  int system = 0;
  int max_reads = 0;
  int max_frames = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream_b = nullptr;  // second demod stream: consecutive calls' demods alternate (LDG_DEMOD_STREAMS)
  int demod_streams = 2;
  hipStream_t stream2 = nullptr;   // frame assembly and output copies, overlapped with the next batch's decode
  hipStream_t scomb = nullptr;     // the fused 2D comb of the assembled frames (own stream: see d_frames)
  hipEvent_t ev_frames = nullptr, ev_comb = nullptr;
  // ldg_output_async's copies, oldest first: ldg_output_wait waits for the oldest
  // outstanding call (the host hands batch k to its sink after issuing batch k+1)
  static constexpr int OUT_Q = 4;
  hipEvent_t ev_outq[OUT_Q] = {};
  int out_head = 0, out_n = 0;
  // decode pipeline: each ldg_decode_reads_async call runs its demod on
  // `stream` (calls in order), its audio phase 2 on `sa` and its field kernel
  // chains split over nsub sub-streams, so one call's field chains (latency
  // bound per read) overlap the next call's demod; up to MAX_CALLS outstanding
  static constexpr int MAX_SUB = 8;
  static constexpr int MAX_CALLS = 8;
  int nsub = 2;                    // LDG_DECODE_STREAMS: 8 measured 15x slower (queue oversubscription), 2 ~ 4
  int stages = 7;                  // debug (LDG_STAGES): bit 0 demod, 1 audio phase 2, 2 field chains
  int skip = 0;                    // debug (LDG_SKIP): field-chain kernels not launched (timing probes only)
  // demod execution spans while profiling (ldg_profile_spans)
  static constexpr int SPAN_MAX = 8192;
  unsigned long long* d_span = nullptr;
  int span_n = 0;
  // host issue time of each profiled demod launch (steady clock, ns) and the
  // calibration that maps it onto the device's constant-rate clock
  std::vector<int64_t> span_issue_ns;
  unsigned long long cal_ticks = 0;
  int64_t cal_ns = 0;
  hipStream_t sub[MAX_SUB] = {};
  hipStream_t sa = nullptr;        // audio phase 2 of each call
  hipStream_t sout = nullptr;      // synchronous output work: 48 kHz audio, field archive
  hipStream_t srec = nullptr;      // each call's field records -> pinned host memory
  // each call's read setup (descriptors into slots, rf filter tables) runs on
  // sprep from pinned host memory, ahead of the previous call's demod finishing
  hipStream_t sprep = nullptr;
  char* h_prep = nullptr;          // [MAX_CALLS] x {ReadDesc[R], int32 smap[R], double mtf[R]}, pinned
  size_t prep_bytes = 0;
  FieldRec* h_recs_pin = nullptr;  // [MAX_CALLS][max_reads], pinned, coherent
  uint64_t* h_done = nullptr;      // [MAX_CALLS] completion sequence numbers (ldg_k_recs_out)
  uint64_t seq = 0;
  struct Call {
    int n = 0;
    std::vector<int32_t> smap;
    hipEvent_t ev_demod = nullptr;
    hipEvent_t ev_done[MAX_SUB + 1] = {};
    hipEvent_t ev_copied = nullptr;  // the call's records are in h_recs_pin
    hipEvent_t ev_prep = nullptr;    // the call's slots and rf tables are set up
    bool demod_recorded = false;     // ev_demod marks the last demod reading this call index's rf tables
    int ndone = 0;
    uint64_t seq = 0;
  };
  Call calls[MAX_CALLS];
  int call_head = 0, ncalls = 0;
  bool frames_recorded = false;    // ev_frames marks the last ldg_assemble_frames (slot readers)
  // pinned staging ring for small host -> device parameter copies
  static constexpr int NSTAGE = 16;
  static constexpr size_t STAGE_BYTES = 1 << 16;
  char* h_stage = nullptr;
  hipEvent_t ev_stage[NSTAGE] = {};
  int stage_next = 0;
  double2* d_ospill = nullptr;     // the demod's odd-spectrum parks, one per physical CU, + owner words
  unsigned long long park_epoch = 0;   // demod launches so far (the parks' owner tags, demod.hip)
  bool comb_pending = false;
  std::string err;
  SysConst C{};
  bool have_filters = false;
  // filter tables (device)
  double2 *tw = nullptr, *rfvideo = nullptr, *mtf = nullptr, *fvideo = nullptr, *f05 = nullptr, *fburst = nullptr,
          *fpilot = nullptr, *fpsync = nullptr, *alf = nullptr, *arf = nullptr, *lpf2 = nullptr;
  double *mtf_logabs = nullptr, *mtf_arg = nullptr;
  double* iirtab = nullptr;       // iir.hpp: FPsync / Fburst / Fpilot coefficients and their powers
  // per call index, one rf filter table per distinct MTF level of the call ([16384],
  // digit-reversed: demod.hip ldg_k_rf_table), grown on demand: a call needs at most
  // its read count of tables, usually a few (CAV: one per frame; CLV: one)
  double2* rf_tab[MAX_CALLS] = {};
  int rf_cap[MAX_CALLS] = {};
  double2* rf_cur = nullptr;      // the tables of the call being launched
  double2* rf_iso = nullptr;      // ldg_demod_isolated_ex's tables (copies of one valid table)
  int rf_iso_cap = 0;
  double2* twk = nullptr;         // twk[p] = W_16384^(dr_nat(p)), p < 8192
  // capture window
  uint8_t* cap = nullptr;
  size_t cap_alloc = 0;
  bool cap_owned = false;
  int64_t cap_first = 0, cap_nsamp = 0;
  int64_t cap_ring = 0;             // > 0: cap is the streamed capture's ring of this many bytes
  CapStream* cs = nullptr;          // the streamed capture (ldg_stream_open), or null
  int fmt = 0;
  // per-read storage
  ReadDesc* d_reads = nullptr;
  int32_t* d_status = nullptr;
  double* video = nullptr;
  int64_t vread = 0, vchan = 0;
  double* audio1 = nullptr;
  int64_t a1read = 0, a1chan = 0;
  double* audio2 = nullptr;
  int64_t a2read = 0, a2chan = 0;
  FieldRec* d_recs = nullptr;
  int32_t* d_peaks = nullptr;
  int32_t *d_npos = nullptr, *d_npk = nullptr, *d_ncnt = nullptr;   // sync-walk segment chains
  double* d_nlv = nullptr;
  double* d_lines = nullptr;
  int8_t* d_bad = nullptr;
  float* d_blevel = nullptr;
  double* d_scratch = nullptr;
  SyncTile* d_stile = nullptr;      // [slot][STILE_PER_SLOT] demod_sync tiles
  double* d_sst = nullptr;          // [slot][CHUNKS_PER_SLOT] compact demod_sync (chan.hpp)
  uint32_t* d_sbits = nullptr;
  double4* d_bst = nullptr;         // [slot][CHUNKS_PER_SLOT] compact demod_burst
  int32_t* d_isomap = nullptr;      // slot map of ldg_demod_isolated
  double2* d_aslice = nullptr;      // [slot][block][2][1024] filtered audio carrier slices
  // pinned host copies of the 48 kHz audio outputs (ldg_field_audio / ldg_archive_audio)
  int16_t* h_pcm = nullptr;
  int32_t* h_counts = nullptr;
  double* h_next = nullptr;
  int32_t* h_aerr = nullptr;
  hipEvent_t ev_audio = nullptr;
  int audio_pending = -1;           // fields of the outstanding ldg_field_audio_async, -1: none
  bool audio_recorded = false;      // ev_audio marks the last audio launch (slot readers)
  uint16_t* d_pic = nullptr;
  int64_t pic_stride = 0;
  std::vector<char> live;           // slot holds a decoded read
  std::vector<ReadDesc> h_reads;
  int32_t* d_smap = nullptr;
  // read-start probes (ldg_k_demod_probe / ldg_k_probe_pick): the probe reads by slot,
  // per call the probed slots, and their pinned host staging
  ReadDesc* d_preads = nullptr;
  int32_t* d_psm = nullptr;        // [MAX_CALLS][R]
  char* h_probe = nullptr;         // [MAX_CALLS] x {ReadDesc[R], int32 slot[R]}, pinned
  int64_t probes = 0;              // probe reads launched (ldg_probe_count)
  // audio / frames staging
  int32_t* d_slots = nullptr;
  int32_t* d_slots2 = nullptr;
  double* d_offsets = nullptr;
  int16_t* d_pcm = nullptr;
  int32_t* d_counts = nullptr;
  double* d_next = nullptr;
  int32_t* d_aerr = nullptr;
  // Two device frame buffers: assembly k + 1 writes one while the comb of batch k
  // (on scomb) still reads the other, so the field chains of later calls, which
  // wait for the last assembly (ev_frames), never wait behind a comb.  fb: the
  // buffer the last assembly wrote; ev_fbuf[b]: after the last reader of buffer b.
  uint16_t* d_frames = nullptr;
  uint16_t* d_frames_b = nullptr;
  int fb = 0;
  bool comb_generic = false;       // LDG_COMB_GENERIC=1: the option-taking comb kernels even at the defaults
  bool comb_unfused = false;       // LDG_COMB_UNFUSED=1: the default 2D comb as three kernels (split, iq, out)
  int comb_iqw = 28;               // ldg_k_comb_fused's FilterIQ exact warm-up after its scan seed (LDG_COMB_IQW, tests)
  int64_t video_cut = 0;           // ldg_set_video_cut: reads' video cut (0: none)
  // RF dropouts (dropout.hip; ldg_set_dropout_opts), allocated when first switched on.
  // Per read slot: what ldg_field_dropouts detects (on sout).  Per field of a frame being
  // assembled (entry 2 f + parity): what the assembly detects and conceals (on stream2).
  bool drop_on = false;
  bool frames_demod = false;       // an assembly has read its slots' demod channel (conceal): the demod waits for ev_frames too
  ldg_dropout_opts drop_opts{};
  int16_t *d_drop_runs = nullptr, *d_fdrop_runs = nullptr;
  int32_t *d_drop_cnt = nullptr, *d_drop_rows = nullptr, *d_fdrop_cnt = nullptr, *d_fdrop_rows = nullptr;
  int32_t *d_drop_map = nullptr, *d_fdrop_map = nullptr;
  char* h_drop = nullptr;          // pinned: the slots' runs, counts and line counts for the host
  // Disc stacking (stack.hip), allocated by the first ldg_stack_frames / ldg_conceal_frames:
  // a stream and buffers of its own, so a decode on this context never sees it.
  hipStream_t sstack = nullptr;
  int stack_cap = 0;               // sources the staging holds
  int64_t stack_src_stride = 0;    // pixels between two sources' frames (a multiple of 8)
  uint16_t *d_stack_src = nullptr, *d_stack_out = nullptr;
  int16_t* d_stack_runs = nullptr;
  int32_t *d_stack_cnt = nullptr, *d_stack_rows = nullptr;
  uint32_t* d_stack_rowinfo = nullptr;   // [max_frames][625]: StackArgs::rowinfo
  double stack_t[4] = {};          // ldg_stack_stats: seconds H2D, kernel, D2H; calls
  ldg_efm_state* efm = nullptr;    // EFM run lengths (efm.hip), allocated by ldg_efm_set_opts
  ldg_efmdec_state* efmdec = nullptr;   // EFM decode (efmdec.hip), allocated by ldg_efmdec_set_table
  ldg_efmsec_state* efmsec = nullptr;   // EFM data sectors (efmsec.hip), allocated on first use
  ldg_lines_state* lines = nullptr;     // NTSC line services (lines.hip), allocated on first use
  ldg_flac_state* flac = nullptr;       // FLAC-compressed capture (flac.hip), allocated by ldg_flac_open
  hipEvent_t ev_fbuf[2] = {nullptr, nullptr};
  bool fbuf_recorded[2] = {false, false};
  hipEvent_t ev_tbc = nullptr;
  uint16_t* frame_buf(int b) const { return b ? d_frames_b : d_frames; }
  // 2D comb state (allocated on first use): aburstlev carried across calls,
  // per-line EMA values of the current call, host-frame staging, rgb48 output
  // field archive (ldg_archive_fields): audio inputs of fields kept past their read slot
  int64_t arch_cap = 0;
  // ldg_archive_audio over more entries than read slots (a rank's whole share at once):
  // its own device and pinned buffers, grown on demand
  struct ArchAudio {
    int64_t cap = 0;
    int64_t* d_idx = nullptr;
    double* d_off = nullptr;
    int16_t* d_pcm = nullptr;
    int32_t* d_counts = nullptr;
    double* d_next = nullptr;
    int32_t* d_err = nullptr;
    char* h = nullptr;             // pinned: idx, off in; pcm, counts, next, err out
  } aa;
  FieldRec* arch_recs = nullptr;
  double* arch_lines = nullptr;
  double* arch_audio2 = nullptr;
  int64_t* d_idx = nullptr;
  std::vector<int64_t> h_idx;
  double* comb_state = nullptr;
  double* comb_abl = nullptr;
  int comb_warm = 5120;             // ldg_k_comb_burst's run-in (LDG_COMB_WARM; tests force the serial fix-up)
  int comb_last_lines = 0;          // lines of the last comb call's burst chain (debug read 50)
  double* comb_cv = nullptr;        // [max_frames][rows][CV_STRIDE] SplitIQ chroma (rows <= 505)
  double* comb_iqo = nullptr;       // [max_frames][iq rows][2][418] FilterIQ outputs
  comb::CombOpt comb_opt = comb_defaults();   // ldg_comb_set_opts
  uint16_t* comb3_win = nullptr;    // 3D: [2 + max_frames] frames, the last two inputs first
  // PAL Y/C decoder (combpal.hip), allocated on first use
  uint16_t *pal_in = nullptr, *pal_rgb = nullptr;
  double *pal_cv = nullptr, *pal_angle = nullptr, *pal_abl = nullptr, *pal_state = nullptr;
  int32_t* pal_phase = nullptr;
  int pal_scur = 0;                 // pal_state[pal_scur]: the burst-level EMA entering the next call
  int pal_last_m = 0;               // frames of the last pal_launch (debug reads 80..84; 0: none yet)
  int comb3_hist = 0;               // 3D: input frames held in the window (0..2)
  // 3D with optical flow (flow.hip): field luma, pyramid, expansions, flows, weight maps
  struct FlowState {
    uint16_t* ybuf = nullptr;                  // [2][FR][FC]
    double *t1 = nullptr, *t2 = nullptr, *I = nullptr, *rows3 = nullptr, *M = nullptr, *V = nullptr;
    double* R[2][3] = {};                      // expansions of the current / previous frame per level
    double* fl[3] = {};                        // flow per level ([2][h][w][2]); level 0 kept across frames
    double* cv2d = nullptr;                    // one frame's 2D chroma rows
    double* kmap = nullptr;                    // weight maps by window slot, [2 + max_frames][FR][FC]
    int rcur = 0;
    int klast = 0;                             // kmap slot of the last flow's weight map (debug read-back)
    int64_t frames = 0;                        // frames the comb has seen (Process calls)
  } of;
  uint16_t* comb_in = nullptr;
  uint16_t* comb_rgb = nullptr;
  double* comb_hist = nullptr;      // -W: DoYNR's last 12 feeds of the previous call, [2][12] (read / write)
  int comb_hist_cur = 0;
  // in-library kernel timing
  bool prof_on = false;
  const char* prof_only = nullptr;  // time only this kernel (ldg_profile_enable mode 2: "demod")
  std::vector<hipEvent_t> prof_pool;
  std::vector<std::pair<std::string, int>> prof_pending;   // name, index of start event
  std::vector<int> prof_free;                               // free event pairs in prof_pool
  std::map<std::string, std::pair<int64_t, double>> prof_stats;
};

namespace {

constexpr int64_t PCM_STRIDE = 2 * 1024;   // int16 per field (>= 2 * 802)
// double2: one demod park per physical CU, the spare and scratch parks, then the owner words
// (PARK_OWNERS x 8 B, demod.hip)
constexpr size_t OSPILL_N = (size_t)PARK_TOTAL * HALF + PARK_OWNERS / 2;

#define LDG_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) {                                                            \
      ctx->err = std::string(#expr) + ": " + hipGetErrorString(e_);                     \
      return LDG_EDEVICE;                                                              \
    }                                                                                  \
  } while (0)

template <class T>
int dmalloc(ldg_ctx* ctx, T** p, size_t count) {
  *p = nullptr;
  if (count == 0) return LDG_OK;
  hipError_t e = hipMalloc((void**)p, count * sizeof(T));
  if (e != hipSuccess) {
    ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e);
    return LDG_ENOMEM;
  }
  return LDG_OK;
}

void dfree(void* p) {
  if (p) (void)hipFree(p);
}

int upload_c128(ldg_ctx* ctx, double2** dst, const double* src, size_t count) {
  if (!src) return LDG_OK;
  if (!*dst) {
    int rc = dmalloc(ctx, dst, count);
    if (rc) return rc;
  }
  LDG_TRY(hipMemcpy(*dst, src, count * sizeof(double2), hipMemcpyHostToDevice));
  return LDG_OK;
}

// A 16384-bin filter (interleaved re, im) reordered for the demod: entry p < M
// holds bin dr_nat(p), entries >= M are unchanged (only bin M is used there).
std::vector<double> dr_order(const double* f) {
  if (!f) return {};   // .data() == nullptr: upload_c128 skips it
  std::vector<double> out(2 * (size_t)BLOCKLEN);
  for (int p = 0; p < BLOCKLEN; p++) {
    const int k = p < HALF ? dr_nat(p) : p;
    out[2 * p] = f[2 * k];
    out[2 * p + 1] = f[2 * k + 1];
  }
  return out;
}

int upload_f64(ldg_ctx* ctx, double** dst, const double* src, size_t count) {
  if (!src) return LDG_OK;
  if (!*dst) {
    int rc = dmalloc(ctx, dst, count);
    if (rc) return rc;
  }
  LDG_TRY(hipMemcpy(*dst, src, count * sizeof(double), hipMemcpyHostToDevice));
  return LDG_OK;
}

int prof_begin(ldg_ctx* ctx, const char* name, hipStream_t st) {
  if (!ctx->prof_on) return -1;
  if (ctx->prof_only && std::strcmp(name, ctx->prof_only)) return -1;
  int k;
  if (!ctx->prof_free.empty()) {
    k = ctx->prof_free.back();
    ctx->prof_free.pop_back();
  } else {
    k = (int)ctx->prof_pool.size();
    for (int j = 0; j < 2; j++) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return -1;
      ctx->prof_pool.push_back(e);
    }
  }
  (void)hipEventRecord(ctx->prof_pool[k], st);
  ctx->prof_pending.push_back({name, k});
  return k;
}

void prof_end(ldg_ctx* ctx, int k, hipStream_t st) {
  if (k >= 0) (void)hipEventRecord(ctx->prof_pool[k + 1], st);
}

// after a stream sync: fold the completed event pairs into the per-kernel
// totals (pairs on the comb stream may still be running: they stay pending;
// pending pairs keep their pool slots, new launches take the next ones)
void prof_collect(ldg_ctx* ctx) {
  std::vector<std::pair<std::string, int>> keep;
  for (auto& pe : ctx->prof_pending) {
    if (hipEventQuery(ctx->prof_pool[pe.second + 1]) == hipErrorNotReady) { keep.push_back(pe); continue; }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->prof_pool[pe.second], ctx->prof_pool[pe.second + 1]) == hipSuccess) {
      auto& st = ctx->prof_stats[pe.first];
      st.first += 1;
      st.second += ms;
    }
    ctx->prof_free.push_back(pe.second);
  }
  ctx->prof_pending.swap(keep);
}

// Copy `bytes` of host memory to the device in stream order through the
// pinned staging ring (the caller's buffer may be reused on return; a ring
// entry is reused only after its previous copy completed).
int stage_h2d(ldg_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t st) {
  if (bytes == 0) return LDG_OK;
  if (bytes > ldg_ctx::STAGE_BYTES) {
    ctx->err = "stage_h2d: parameter block too large";
    return LDG_EINVAL;
  }
  const int k = ctx->stage_next;
  ctx->stage_next = (k + 1) % ldg_ctx::NSTAGE;
  LDG_TRY(hipEventSynchronize(ctx->ev_stage[k]));
  char* h = ctx->h_stage + (size_t)k * ldg_ctx::STAGE_BYTES;
  std::memcpy(h, src, bytes);
  LDG_TRY(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, st));
  LDG_TRY(hipEventRecord(ctx->ev_stage[k], st));
  return LDG_OK;
}

#define LDG_LAUNCH_ON(ST, NAME, KERNEL, GRID, BLOCK, ...)     \
  do {                                                        \
    const int pi_ = prof_begin(ctx, NAME, ST);                \
    KERNEL<<<GRID, BLOCK, 0, ST>>>(__VA_ARGS__);              \
    prof_end(ctx, pi_, ST);                                   \
  } while (0)
#define LDG_LAUNCH(NAME, KERNEL, GRID, BLOCK, ...) LDG_LAUNCH_ON(ctx->stream, NAME, KERNEL, GRID, BLOCK, __VA_ARGS__)

int check_launch(ldg_ctx* ctx, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return LDG_EDEVICE;
  }
  return LDG_OK;
}

// ldg_k_stack unrolled for N source slots (stack.hip)
template <int N>
void stack_launch(ldg_ctx* ctx, hipStream_t s, dim3 grid, const StackArgs& A) {
  LDG_LAUNCH_ON(s, "stack", ldg_k_stack<N>, grid, STACK_THREADS, A);
}

// a call's read descriptors (pinned host memory) into their slots; the slot
// map to the device; clear the slots' status words
__global__ void ldg_k_new_reads(const ReadDesc* __restrict__ src, const int32_t* __restrict__ smap, int n,
                                int32_t* __restrict__ dsmap, ReadDesc* __restrict__ reads, int32_t* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const int32_t sl = smap[i];
    dsmap[i] = sl;
    reads[sl] = src[i];
    status[sl] = 0;
  }
}

// the records of a call's slots, in call order, to pinned host memory (a
// kernel, not a DMA copy: the copy engine's cross-queue start latency is
// hundreds of microseconds, which the next call's launch would wait out)
// One workgroup; after the records it stores `seq` to *flag (system scope),
// which the host polls: an event wait takes as long again to notice.  It also
// ends the field analysis (formerly a per-group kernel): records still
// pending after the TBC pass become FS_VALID, in HBM and in the copy.
__global__ void __launch_bounds__(256) ldg_k_recs_out(FieldRec* __restrict__ recs,
                                                      const int32_t* __restrict__ smap, int n,
                                                      const ReadDesc* __restrict__ reads,
                                                      FieldRec* __restrict__ out, uint64_t* flag, uint64_t seq) {
  static_assert(sizeof(FieldRec) % 4 == 0, "FieldRec words");
  constexpr int W = sizeof(FieldRec) / 4;
  for (int i = threadIdx.x; i < n; i += 256) {
    FieldRec* r = recs + smap[i];
    if (r->status == FS_PENDING) r->status = FS_VALID;
    r->readsample = reads[smap[i]].readsample;     // a start probe may have moved it
  }
  __syncthreads();
  for (int i = threadIdx.x / 64; i < n; i += 4) {
    const uint32_t* src = (const uint32_t*)(recs + smap[i]);
    uint32_t* dst = (uint32_t*)(out + i);
    for (int w = threadIdx.x & 63; w < W; w += 64) dst[w] = src[w];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence_system();
    __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ldg_archive_fields' copies in one launch: field i (slot slots[i]) into archive
// entry first + i -- its record, its final line locations and its audio phase-2
// samples.  grid: (chunks, n) workgroups of 256 threads.
__global__ void __launch_bounds__(256) ldg_k_archive(const int64_t* __restrict__ slots, int64_t first,
                                                     const FieldRec* __restrict__ recs, const double* __restrict__ lines,
                                                     const double* __restrict__ audio2, int64_t a2read,
                                                     FieldRec* __restrict__ arecs, double* __restrict__ alines,
                                                     double* __restrict__ aaudio2) {
  constexpr int W = sizeof(FieldRec) / 4;
  const int64_t sl = slots[blockIdx.y], e = first + blockIdx.y;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  if (blockIdx.x == 0 && threadIdx.x < W)
    ((uint32_t*)(arecs + e))[threadIdx.x] = ((const uint32_t*)(recs + sl))[threadIdx.x];
  const double* ls = lines + sl * LINES_STRIDE + LLF * MAX_LINES;
  for (int64_t k = tid; k < MAX_LINES; k += step) alines[e * MAX_LINES + k] = ls[k];
  const double* as = audio2 + sl * a2read;
  for (int64_t k = tid; k < a2read; k += step) aaudio2[e * a2read + k] = as[k];
}

}  // namespace

extern "C" {

const char* ldg_version(void) { return "ldgpu 0.1 (gfx950)"; }

int ldg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int ldg_device_memory(int device, int64_t* free_bytes, int64_t* total_bytes) {
  if (!free_bytes || !total_bytes) return LDG_EINVAL;
  size_t f = 0, t = 0;
  if (hipSetDevice(device) != hipSuccess || hipMemGetInfo(&f, &t) != hipSuccess) return LDG_EDEVICE;
  *free_bytes = (int64_t)f;
  *total_bytes = (int64_t)t;
  return LDG_OK;
}

const char* ldg_last_error(const ldg_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int ldg_create(const ldg_config* cfg, ldg_ctx** out) {
  if (!cfg || !out || cfg->max_reads <= 0 || (cfg->system != 0 && cfg->system != 1)) return LDG_EINVAL;
  *out = nullptr;
  ldg_ctx* ctx = new ldg_ctx();
  ctx->device = cfg->device;
  ctx->system = cfg->system;
  ctx->max_reads = cfg->max_reads;
  ctx->max_frames = cfg->max_frames > 0 ? cfg->max_frames : cfg->max_reads;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) {
    delete ctx;
    return LDG_EDEVICE;
  }
  if (const char* e = getenv("LDG_DEMOD_STREAMS")) ctx->demod_streams = atoi(e) == 1 ? 1 : 2;
  if (const char* e = getenv("LDG_COMB_GENERIC")) ctx->comb_generic = atoi(e) != 0;
  if (const char* e = getenv("LDG_COMB_UNFUSED")) ctx->comb_unfused = atoi(e) != 0;
  if (const char* e = getenv("LDG_COMB_IQW")) ctx->comb_iqw = std::max(0, atoi(e));
  if (const char* e = getenv("LDG_COMB_WARM")) ctx->comb_warm = std::max(0, atoi(e));
  if (const char* e = getenv("LDG_DECODE_STREAMS")) ctx->nsub = atoi(e);
  ctx->nsub = ctx->nsub < 1 ? 1 : ctx->nsub > ldg_ctx::MAX_SUB ? ldg_ctx::MAX_SUB : ctx->nsub;
  // Streams in creation order, which is the order of their hardware queues. It
  // matters: over 20 sustained steps the round-3 order (output and comb streams
  // second and third) ran 96.2 ms per 60 s step, the round-2 order (comb last)
  // 94.4, and orders that create the demod and field-chain streams first 91.5 –
  // 92.7 (profiles/r03_k_stream_order.txt).
  bool made_ok = true;
  auto make = [&](hipStream_t* st) { made_ok &= hipStreamCreateWithFlags(st, hipStreamNonBlocking) == hipSuccess; };
  make(&ctx->stream);                                        // D demod
  for (int k = 0; k < ctx->nsub; k++) make(&ctx->sub[k]);    // S the field-chain streams
  make(&ctx->stream_b);                                      // d second demod
  make(&ctx->sa);                                            // a audio
  make(&ctx->stream2);                                       // o output
  make(&ctx->sout);                                          // s audio out
  make(&ctx->srec);                                          // r records
  make(&ctx->sprep);                                         // p read setup
  make(&ctx->scomb);                                         // c comb
  if (!made_ok ||
      hipEventCreateWithFlags(&ctx->ev_fbuf[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_fbuf[1], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_tbc, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_frames, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_outq[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_outq[1], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_outq[2], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_outq[3], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_comb, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_audio, hipEventDisableTiming) != hipSuccess ||
      hipHostMalloc((void**)&ctx->h_stage, ldg_ctx::NSTAGE * ldg_ctx::STAGE_BYTES, hipHostMallocDefault) != hipSuccess) {
    ldg_destroy(ctx);
    return LDG_EDEVICE;
  }
  for (int k = 0; k < ldg_ctx::NSTAGE; k++)
    if (hipEventCreateWithFlags(&ctx->ev_stage[k], hipEventDisableTiming) != hipSuccess) {
      ldg_destroy(ctx);
      return LDG_EDEVICE;
    }
  for (auto& c : ctx->calls) {
    if (hipEventCreateWithFlags(&c.ev_demod, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c.ev_copied, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c.ev_prep, hipEventDisableTiming) != hipSuccess) {
      ldg_destroy(ctx);
      return LDG_EDEVICE;
    }
    for (auto& e : c.ev_done)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
        ldg_destroy(ctx);
        return LDG_EDEVICE;
      }
  }
  const int R = ctx->max_reads;
  const int nchan = ctx->system == 1 ? 5 : 4;
  ctx->vchan = MAX_NOUT;
  ctx->vread = (int64_t)nchan * MAX_NOUT;
  ctx->a1chan = MAX_NAUDIO;
  ctx->a1read = 2 * MAX_NAUDIO;
  ctx->a2chan = MAX_NAUDIO2;
  ctx->a2read = 2 * MAX_NAUDIO2;
  ctx->pic_stride = (int64_t)MAX_LINES * MAX_OUTW;
  int rc = 0;
  rc |= dmalloc(ctx, &ctx->d_reads, R);
  rc |= dmalloc(ctx, &ctx->d_smap, (size_t)ldg_ctx::MAX_CALLS * R);
  rc |= dmalloc(ctx, &ctx->d_preads, (size_t)R);
  rc |= dmalloc(ctx, &ctx->d_psm, (size_t)ldg_ctx::MAX_CALLS * R);
  ctx->live.assign(R, 0);
  rc |= dmalloc(ctx, &ctx->d_status, R);
  rc |= dmalloc(ctx, &ctx->video, (size_t)R * ctx->vread);
  rc |= dmalloc(ctx, &ctx->audio1, (size_t)R * ctx->a1read);
  rc |= dmalloc(ctx, &ctx->audio2, (size_t)R * ctx->a2read);
  rc |= dmalloc(ctx, &ctx->d_recs, R);
  rc |= dmalloc(ctx, &ctx->d_peaks, (size_t)R * MAX_PEAKS);
  rc |= dmalloc(ctx, &ctx->d_npos, (size_t)R * SEG_K * SEG_NMAX);
  rc |= dmalloc(ctx, &ctx->d_npk, (size_t)R * SEG_K * SEG_NMAX);
  rc |= dmalloc(ctx, &ctx->d_nlv, (size_t)R * SEG_K * SEG_NMAX);
  rc |= dmalloc(ctx, &ctx->d_ncnt, (size_t)R * SEG_K);
  rc |= dmalloc(ctx, &ctx->d_lines, (size_t)R * LINES_STRIDE);
  rc |= dmalloc(ctx, &ctx->d_bad, (size_t)R * MAX_LINES);
  rc |= dmalloc(ctx, &ctx->d_blevel, (size_t)R * MAX_LINES);
  // the demod's odd-spectrum park (10 x 1024 double2 per block, per batch
  // position) and the PAL pilot scratch (per slot)
  rc |= dmalloc(ctx, &ctx->d_ospill, OSPILL_N);
  // the parks' owner words start free (0; tags are >= 1 << 32)
  if (!rc && hipMemset(ctx->d_ospill + (size_t)PARK_TOTAL * HALF, 0, (size_t)PARK_OWNERS * 8) != hipSuccess)
    rc |= LDG_EDEVICE;
  rc |= dmalloc(ctx, &ctx->d_scratch, (size_t)R * SCR_PER_SLOT);
  rc |= dmalloc(ctx, &ctx->d_stile, (size_t)R * STILE_PER_SLOT);
  rc |= dmalloc(ctx, &ctx->d_sst, (size_t)R * CHUNKS_PER_SLOT);
  rc |= dmalloc(ctx, &ctx->d_sbits, (size_t)R * CHUNKS_PER_SLOT);
  rc |= dmalloc(ctx, &ctx->d_bst, (size_t)R * CHUNKS_PER_SLOT);
  rc |= dmalloc(ctx, &ctx->d_aslice, (size_t)R * MAX_BLOCKS_PER_READ * 2048);
  ctx->prep_bytes = (size_t)R * (sizeof(ReadDesc) + sizeof(int32_t) + sizeof(double));
  if (hipHostMalloc((void**)&ctx->h_prep, ldg_ctx::MAX_CALLS * ctx->prep_bytes, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&ctx->h_probe, ldg_ctx::MAX_CALLS * (size_t)R * (sizeof(ReadDesc) + sizeof(int32_t)),
                    hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&ctx->h_recs_pin, (size_t)ldg_ctx::MAX_CALLS * R * sizeof(FieldRec),
                    hipHostMallocCoherent) != hipSuccess ||
      hipHostMalloc((void**)&ctx->h_done, ldg_ctx::MAX_CALLS * sizeof(uint64_t), hipHostMallocCoherent) != hipSuccess ||
      hipHostMalloc((void**)&ctx->h_pcm, (size_t)R * PCM_STRIDE * sizeof(int16_t), hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&ctx->h_counts, (size_t)R * sizeof(int32_t), hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&ctx->h_next, (size_t)R * sizeof(double), hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&ctx->h_aerr, (size_t)R * sizeof(int32_t), hipHostMallocDefault) != hipSuccess)
    rc |= LDG_ENOMEM;
  if (ctx->h_done) std::memset(ctx->h_done, 0, ldg_ctx::MAX_CALLS * sizeof(uint64_t));
  rc |= dmalloc(ctx, &ctx->d_pic, (size_t)R * ctx->pic_stride);
  rc |= dmalloc(ctx, &ctx->d_slots, R);
  rc |= dmalloc(ctx, &ctx->d_slots2, R);
  rc |= dmalloc(ctx, &ctx->d_offsets, R);
  rc |= dmalloc(ctx, &ctx->d_idx, R);
  rc |= dmalloc(ctx, &ctx->d_pcm, (size_t)R * PCM_STRIDE);
  rc |= dmalloc(ctx, &ctx->d_counts, R);
  rc |= dmalloc(ctx, &ctx->d_next, R);
  rc |= dmalloc(ctx, &ctx->d_aerr, R);
  rc |= dmalloc(ctx, &ctx->d_frames, (size_t)ctx->max_frames * 625 * MAX_OUTW);
  rc |= dmalloc(ctx, &ctx->d_frames_b, (size_t)ctx->max_frames * 625 * MAX_OUTW);
  if (rc) {
    ldg_destroy(ctx);
    return LDG_ENOMEM;
  }
  // twiddles W[m] = exp(-2 pi i m / 16384)
  std::vector<double2> tw(TW_N);
  for (int m = 0; m < TW_N; m++) {
    const long double a = -2.0L * 3.141592653589793238462643383279502884L * (long double)m / (long double)TW_N;
    tw[m] = make_double2((double)cosl(a), (double)sinl(a));
  }
  std::vector<double2> twk(HALF);
  for (int p = 0; p < HALF; p++) twk[p] = tw[dr_nat(p)];
  if (dmalloc(ctx, &ctx->tw, TW_N) || hipMemcpy(ctx->tw, tw.data(), TW_N * sizeof(double2), hipMemcpyHostToDevice) ||
      dmalloc(ctx, &ctx->twk, HALF) || hipMemcpy(ctx->twk, twk.data(), HALF * sizeof(double2), hipMemcpyHostToDevice)) {
    ldg_destroy(ctx);
    return LDG_EDEVICE;
  }
  *out = ctx;
  return LDG_OK;
}

static void arch_audio_free(ldg_ctx* ctx);
static void stack_free(ldg_ctx* ctx);
static void efm_free(ldg_ctx* ctx);   // efm.inc
static void efmdec_free(ldg_ctx* ctx);   // efmdec.inc
static void efmsec_free(ldg_ctx* ctx);   // efmsec.inc
static void lines_free(ldg_ctx* ctx);    // lines.inc
static void flac_free(ldg_ctx* ctx);     // flac.inc

int ldg_destroy(ldg_ctx* ctx) {
  if (!ctx) return LDG_EINVAL;
  (void)hipSetDevice(ctx->device);
  (void)ldg_stream_close(ctx);
  for (hipStream_t st : {ctx->stream, ctx->stream_b, ctx->stream2, ctx->scomb, ctx->sa, ctx->sout, ctx->srec, ctx->sprep})
    if (st) (void)hipStreamSynchronize(st);
  for (int k = 0; k < ldg_ctx::MAX_SUB; k++)
    if (ctx->sub[k]) {
      (void)hipStreamSynchronize(ctx->sub[k]);
      (void)hipStreamDestroy(ctx->sub[k]);
    }
  for (auto& c : ctx->calls) {
    if (c.ev_demod) (void)hipEventDestroy(c.ev_demod);
    if (c.ev_copied) (void)hipEventDestroy(c.ev_copied);
    if (c.ev_prep) (void)hipEventDestroy(c.ev_prep);
    for (auto e : c.ev_done)
      if (e) (void)hipEventDestroy(e);
  }
  for (auto e : ctx->ev_stage)
    if (e) (void)hipEventDestroy(e);
  if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
  dfree(ctx->d_stile);
  dfree(ctx->d_sst);
  dfree(ctx->d_sbits);
  dfree(ctx->d_bst);
  dfree(ctx->d_isomap);
  dfree(ctx->d_aslice);
  dfree(ctx->d_preads);
  dfree(ctx->d_psm);
  for (void* h : {(void*)ctx->h_pcm, (void*)ctx->h_counts, (void*)ctx->h_next, (void*)ctx->h_aerr})
    if (h) (void)hipHostFree(h);
  dfree(ctx->d_ospill);
  void* ps[] = {ctx->tw, ctx->twk, ctx->rfvideo, ctx->mtf, ctx->fvideo, ctx->f05, ctx->fburst, ctx->fpilot, ctx->fpsync,
                ctx->alf, ctx->arf, ctx->lpf2, ctx->mtf_logabs, ctx->mtf_arg, ctx->iirtab, ctx->rf_iso, ctx->d_reads, ctx->d_smap,
                ctx->d_status, ctx->video, ctx->audio1, ctx->audio2, ctx->d_recs, ctx->d_peaks, ctx->d_npos, ctx->d_npk, ctx->d_nlv, ctx->d_ncnt, ctx->d_lines,
                ctx->d_bad, ctx->d_blevel, ctx->d_scratch, ctx->d_pic, ctx->d_slots, ctx->d_slots2, ctx->d_offsets,
                ctx->d_pcm, ctx->d_counts, ctx->d_next, ctx->d_aerr, ctx->d_frames, ctx->d_frames_b};
  for (void* p : ps) dfree(p);
  for (double2* t : ctx->rf_tab) dfree(t);
  for (void* p : {(void*)ctx->d_drop_runs, (void*)ctx->d_fdrop_runs, (void*)ctx->d_drop_cnt, (void*)ctx->d_drop_rows,
                  (void*)ctx->d_fdrop_cnt, (void*)ctx->d_fdrop_rows, (void*)ctx->d_drop_map, (void*)ctx->d_fdrop_map})
    dfree(p);
  if (ctx->h_drop) (void)hipHostFree(ctx->h_drop);
  stack_free(ctx);
  efm_free(ctx);
  efmdec_free(ctx);
  efmsec_free(ctx);
  lines_free(ctx);
  flac_free(ctx);
  if (ctx->cap_owned) dfree(ctx->cap);

  for (void* p : {(void*)ctx->comb_state, (void*)ctx->comb_abl, (void*)ctx->comb_in, (void*)ctx->comb_rgb,
                  (void*)ctx->comb3_win, (void*)ctx->d_span, (void*)ctx->pal_in, (void*)ctx->pal_rgb, (void*)ctx->pal_cv,
                  (void*)ctx->pal_angle, (void*)ctx->pal_abl, (void*)ctx->pal_state, (void*)ctx->pal_phase,
                  (void*)ctx->comb_cv, (void*)ctx->comb_iqo, (void*)ctx->comb_hist,
                  (void*)ctx->arch_recs, (void*)ctx->arch_lines, (void*)ctx->arch_audio2, (void*)ctx->d_idx})
    dfree(p);
  {
    auto& F = ctx->of;
    for (void* p : {(void*)F.ybuf, (void*)F.t1, (void*)F.t2, (void*)F.I, (void*)F.rows3, (void*)F.M, (void*)F.V,
                    (void*)F.cv2d, (void*)F.kmap})
      dfree(p);
    for (auto& rr : F.R)
      for (double* p : rr) dfree(p);
    for (double* p : F.fl) dfree(p);
  }
  for (hipEvent_t e : ctx->prof_pool) (void)hipEventDestroy(e);
  for (hipStream_t st : {ctx->stream, ctx->stream_b, ctx->stream2, ctx->scomb, ctx->sa, ctx->sout, ctx->srec, ctx->sprep})
    if (st) (void)hipStreamDestroy(st);
  if (ctx->h_recs_pin) (void)hipHostFree(ctx->h_recs_pin);
  if (ctx->h_prep) (void)hipHostFree(ctx->h_prep);
  if (ctx->h_probe) (void)hipHostFree(ctx->h_probe);
  arch_audio_free(ctx);
  if (ctx->h_done) (void)hipHostFree(ctx->h_done);
  if (ctx->ev_frames) (void)hipEventDestroy(ctx->ev_frames);
  for (hipEvent_t e : ctx->ev_outq)
    if (e) (void)hipEventDestroy(e);
  if (ctx->ev_comb) (void)hipEventDestroy(ctx->ev_comb);
  for (hipEvent_t e : {ctx->ev_fbuf[0], ctx->ev_fbuf[1], ctx->ev_tbc})
    if (e) (void)hipEventDestroy(e);
  if (ctx->ev_audio) (void)hipEventDestroy(ctx->ev_audio);
  delete ctx;
  return LDG_OK;
}

// The time-domain filter table of iir.hpp from the butter(1) coefficients behind
// fpsync, Fburst and Fpilot (ldg_filters.iir), after checking that the sampled
// responses the caller passed are those filters: fpsync[k] = B/A(w_k) and
// fvideoburst[k] = fvideo[k] * B/A(w_k) (lddecode_core.py:204-214).
static int build_iir(ldg_ctx* ctx, const ldg_filters* f, std::vector<double>& tab) {
  if (!f->iir) {
    ctx->err = "ldg_filters.iir (FPsync / Fburst / Fpilot coefficients) is required";
    return LDG_EINVAL;
  }
  tab.assign(IIR_TAB_N, 0.0);
  for (int i = 0; i < IIR_NCOEF; i++) tab[i] = f->iir[i];
  // the sync recurrence (iir.hpp sync_step) computes b0 * (x + x_prev): butter(1)'s b1 == b0
  if (tab[1] != tab[0]) {
    ctx->err = "ldg_filters.iir: FPsync must have b1 == b0 (a first-order Butterworth low pass)";
    return LDG_EINVAL;
  }
  auto resp = [](const double* b, const double* a, int nb, int k) {   // B/A at w_k = 2 pi k / N
    std::complex<double> z = std::polar(1.0, -2.0 * M_PI * k / BLOCKLEN), num = 0, den = 0, zp = 1;
    for (int i = 0; i < nb; i++) { num += b[i] * zp; den += a[i] * zp; zp *= z; }
    return num / den;
  };
  const double a_ps[2] = {1.0, tab[2]}, a_b[3] = {1.0, tab[6], tab[7]}, a_p[3] = {1.0, tab[11], tab[12]};
  auto c = [](const double* v, int k) { return std::complex<double>(v[2 * k], v[2 * k + 1]); };
  double e_ps = 0, e_b = 0, e_p = 0, m_ps = 0, m_b = 0, m_p = 0;
  for (int k = 0; k < BLOCKLEN; k++) {
    e_ps = std::max(e_ps, std::abs(c(f->fpsync, k) - resp(tab.data(), a_ps, 2, k)));
    m_ps = std::max(m_ps, std::abs(c(f->fpsync, k)));
    e_b = std::max(e_b, std::abs(c(f->fvideoburst, k) - c(f->fvideo, k) * resp(tab.data() + 3, a_b, 3, k)));
    m_b = std::max(m_b, std::abs(c(f->fvideoburst, k)));
    if (ctx->system == 1 && f->fvideopilot) {
      e_p = std::max(e_p, std::abs(c(f->fvideopilot, k) - c(f->fvideo, k) * resp(tab.data() + 8, a_p, 3, k)));
      m_p = std::max(m_p, std::abs(c(f->fvideopilot, k)));
    }
  }
  if (e_ps > 1e-9 * m_ps || e_b > 1e-9 * m_b || e_p > 1e-9 * m_p || (ctx->system == 1 && !f->fvideopilot)) {
    char buf[160];
    snprintf(buf, sizeof buf, "ldg_filters.iir does not match the sampled filters (rel. err psync %.2g burst %.2g pilot %.2g)",
             e_ps / std::max(m_ps, 1e-300), e_b / std::max(m_b, 1e-300), e_p / std::max(m_p, 1e-300));
    ctx->err = buf;
    return LDG_EINVAL;
  }
  // the F05 FIR, when given: fvideo05 must be fvideo * DFT(taps) on every bin (a
  // cross-check of the caller's filter set; the demod applies fvideo05 itself)
  if (f->f05_fir) {
    constexpr int F05_TAPS = 65;
    double e = 0, m = 0;
    for (int k = 0; k < BLOCKLEN; k++) {
      std::complex<double> h = 0;
      for (int j = 0; j < F05_TAPS; j++) h += f->f05_fir[j] * std::polar(1.0, -2.0 * M_PI * (double)((int64_t)j * k % BLOCKLEN) / BLOCKLEN);
      e = std::max(e, std::abs(c(f->fvideo05, k) - c(f->fvideo, k) * h));
      m = std::max(m, std::abs(c(f->fvideo05, k)));
    }
    if (e > 1e-9 * m) {
      char buf[120];
      snprintf(buf, sizeof buf, "ldg_filters.f05_fir does not match fvideo05 / fvideo (rel. err %.2g)", e / std::max(m, 1e-300));
      ctx->err = buf;
      return LDG_EINVAL;
    }
  }
  // p^(16 s) of FPsync (p = -a1)
  {
    double p16 = 1.0;
    for (int i = 0; i < IIR_CHUNK; i++) p16 *= -tab[2];
    tab[IIR_P1] = 1.0;
    for (int s = 1; s < IIR_NPOW; s++) tab[IIR_P1 + s] = tab[IIR_P1 + s - 1] * p16;
  }
  // C^(16 s) of the second-order sections, C = [[-a1, -a2], [1, 0]]
  for (int sec = 0; sec < 2; sec++) {
    const double a1 = tab[sec ? 11 : 6], a2 = tab[sec ? 12 : 7];
    double* M = tab.data() + (sec ? IIR_MP : IIR_MB);
    double c16[4] = {1, 0, 0, 1};
    for (int i = 0; i < IIR_CHUNK; i++) {
      const double r[4] = {-a1 * c16[0] - a2 * c16[2], -a1 * c16[1] - a2 * c16[3], c16[0], c16[1]};
      for (int j = 0; j < 4; j++) c16[j] = r[j];
    }
    M[0] = 1; M[1] = 0; M[2] = 0; M[3] = 1;
    for (int s = 1; s < IIR_NPOW; s++) {
      const double* P = M + 4 * (s - 1);
      double* Q = M + 4 * s;
      Q[0] = P[0] * c16[0] + P[1] * c16[2];
      Q[1] = P[0] * c16[1] + P[1] * c16[3];
      Q[2] = P[2] * c16[0] + P[3] * c16[2];
      Q[3] = P[2] * c16[1] + P[3] * c16[3];
    }
  }
  return LDG_OK;
}

int ldg_set_filters(ldg_ctx* ctx, const ldg_params* p, const ldg_filters* f) {
  if (!ctx || !p || !f) return LDG_EINVAL;
  LDG_TRY(hipSetDevice(ctx->device));
  SysConst& C = ctx->C;
  C.freq_hz = p->freq_hz; C.freq = p->freq; C.ire0 = p->ire0; C.hz_ire = p->hz_ire; C.vsync_ire = p->vsync_ire;
  C.sync_lo = p->sync_lo; C.sync_hi = p->sync_hi; C.freq_arf = p->freq_arf; C.audio_lowfreq = p->audio_lowfreq;
  C.audio_lfreq = p->audio_lfreq; C.audio_rfreq = p->audio_rfreq; C.line_period = p->line_period;
  C.fsc_mhz = p->fsc_mhz; C.system = ctx->system; C.linelen = p->linelen; C.outlinelen = p->outlinelen;
  C.frame_lines = p->frame_lines; C.n_chan = ctx->system == 1 ? 5 : 4; C.audio_lo0 = p->audio_lo0;
  for (int i = 0; i < 3; i++) C.codelines[i] = p->codelines[i];
  if (C.outlinelen > MAX_OUTW || C.linelen + 200 >= 2816) { ctx->err = "unsupported line geometry"; return LDG_EINVAL; }
  // tbc_pixel's per-context constants, by the divisions the kernel made per pixel (the same bits)
  C.hz_ire_r = divconst_ok(C.hz_ire) ? 1.0 / C.hz_ire : 0.0;
  C.tbc_scale = (ctx->system == 1 ? (double)(0xd300 - 0x0100) : (double)(0xc800 - 0x0400)) / (100 - C.vsync_ire);
  int rc = 0;
  rc |= upload_c128(ctx, &ctx->rfvideo, f->rfvideo, BLOCKLEN);
  rc |= upload_c128(ctx, &ctx->mtf, f->mtf, BLOCKLEN);
  // the output filters in the demod's digit-reversed bin order (bins 0..M used)
  rc |= upload_c128(ctx, &ctx->fvideo, dr_order(f->fvideo).data(), BLOCKLEN);
  rc |= upload_c128(ctx, &ctx->f05, dr_order(f->fvideo05).data(), BLOCKLEN);
  rc |= upload_c128(ctx, &ctx->fburst, dr_order(f->fvideoburst).data(), BLOCKLEN);
  rc |= upload_c128(ctx, &ctx->fpilot, dr_order(f->fvideopilot ? f->fvideopilot : f->fvideo).data(), BLOCKLEN);
  rc |= upload_c128(ctx, &ctx->fpsync, dr_order(f->fpsync).data(), BLOCKLEN);
  rc |= upload_c128(ctx, &ctx->alf, f->audio_lfilt, AUDIO_BLOCK);
  rc |= upload_c128(ctx, &ctx->arf, f->audio_rfilt, AUDIO_BLOCK);
  rc |= upload_c128(ctx, &ctx->lpf2, f->audio_lpf2, AUDIO2_BLOCK);
  rc |= upload_f64(ctx, &ctx->mtf_logabs, f->mtf_logabs, BLOCKLEN);
  rc |= upload_f64(ctx, &ctx->mtf_arg, f->mtf_arg, BLOCKLEN);
  if (rc) return rc;
  std::vector<double> iirtab;
  if (int e = build_iir(ctx, f, iirtab)) return e;
  C.sy_b0 = iirtab[0];
  C.sy_p = -iirtab[2];
  C.bu_b0 = iirtab[3]; C.bu_b1 = iirtab[4]; C.bu_b2 = iirtab[5]; C.bu_a1 = iirtab[6]; C.bu_a2 = iirtab[7];
  rc |= upload_f64(ctx, &ctx->iirtab, iirtab.data(), IIR_TAB_N);
  if (rc) return rc;
  ctx->have_filters = true;
  return LDG_OK;
}

int ldg_set_capture(ldg_ctx* ctx, const void* data, int64_t nsamples, int fmt, int64_t first_sample,
                    int is_device) {
  if (!ctx || !data || nsamples <= 0 || fmt < 0 || fmt > 3 || first_sample < 0) return LDG_EINVAL;
  if ((fmt == 2 && first_sample % 3) || (fmt == 3 && first_sample % 4)) return LDG_EINVAL;
  LDG_TRY(hipSetDevice(ctx->device));
  if (int rc = ldg_stream_close(ctx)) return rc;      // a resident capture replaces a streamed one
  ctx->cap_ring = 0;
  size_t nbytes;
  switch (fmt) {
    case 0: nbytes = (size_t)nsamples; break;
    case 1: nbytes = (size_t)nsamples * 2; break;
    case 2: nbytes = (size_t)((nsamples + 2) / 3) * 4; break;
    default: nbytes = (size_t)((nsamples + 3) / 4) * 5; break;
  }
  if (is_device) {
    if (ctx->cap_owned) dfree(ctx->cap);
    ctx->cap = (uint8_t*)data;
    ctx->cap_owned = false;
    ctx->cap_alloc = nbytes;
  } else {
    if (!ctx->cap_owned || ctx->cap_alloc < nbytes) {
      if (ctx->cap_owned) dfree(ctx->cap);
      ctx->cap = nullptr;
      int rc = dmalloc(ctx, &ctx->cap, nbytes + 16);
      if (rc) return rc;
      ctx->cap_alloc = nbytes;
      ctx->cap_owned = true;
    }
    LDG_TRY(hipMemcpy(ctx->cap, data, nbytes, hipMemcpyHostToDevice));
  }
  ctx->fmt = fmt;
  ctx->cap_first = first_sample;
  ctx->cap_nsamp = nsamples;
  return LDG_OK;
}

static int stream_prepare(ldg_ctx* ctx, hipStream_t s, int64_t hi);   // stream.inc

// Profiling: the next demod launch's execution-span slot ({max ~start, max end}
// on the device's constant-rate clock, zero-initialised), or null when not
// profiling / full.
static int64_t steady_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}
static unsigned long long* span_slot(ldg_ctx* ctx) {
  if (!ctx->prof_on || !ctx->d_span || ctx->span_n >= ldg_ctx::SPAN_MAX) return nullptr;
  ctx->span_issue_ns.push_back(steady_ns());   // evaluated as the launch's argument: its issue time
  return ctx->d_span + 2 * (size_t)ctx->span_n++;
}

// The demod of the n reads whose slots are M_[0..n), on stream st.
static int launch_demod(ldg_ctx* ctx, hipStream_t st, int n, const int32_t* M_) {
  const SysConst C = ctx->C;
  LDG_LAUNCH_ON(st, "demod", ldg_k_demod, n * MAX_BLOCKS_PER_READ, 1024, M_, ctx->d_reads, ctx->cap, ctx->cap_first,
             ctx->cap_nsamp, ctx->cap_ring, ctx->fmt, ctx->tw, ctx->twk, ctx->rf_cur, ctx->fvideo, ctx->f05, ctx->iirtab, ctx->alf, ctx->arf, C, ctx->video, ctx->vread, ctx->vchan,
             ctx->d_status, ctx->d_ospill, ++ctx->park_epoch, ctx->d_stile, ctx->d_aslice,
             ctx->d_sst, ctx->d_sbits, ctx->d_bst, span_slot(ctx));
  return check_launch(ctx, "ldg_k_demod");
}

// The per-read field kernel chain (sync -> line locations -> TBC) for n demodulated
// reads whose slots are M_[0..n), on stream st.
static int launch_chain(ldg_ctx* ctx, hipStream_t st, int n, const int32_t* M_) {
  const SysConst C = ctx->C;
  if (!(ctx->skip >> 0 & 1)) LDG_LAUNCH_ON(st, "sync_walk", ldg_k_sync_walk, n * SEG_K, 64, M_, ctx->d_reads, ctx->video, ctx->vread, ctx->vchan, C,
             ctx->d_status, ctx->d_npos, ctx->d_npk, ctx->d_nlv, ctx->d_ncnt, ctx->d_stile, ctx->d_sst,
             ctx->d_sbits);
  if (!(ctx->skip >> 1 & 1)) LDG_LAUNCH_ON(st, "sync", ldg_k_sync, n, 64, M_, ctx->d_reads, ctx->video, ctx->vread, ctx->vchan, C, ctx->d_recs,
             ctx->d_peaks, ctx->d_status, ctx->d_npos, ctx->d_npk, ctx->d_nlv, ctx->d_ncnt, ctx->d_stile,
             ctx->d_sst, ctx->d_sbits, (ctx->skip >> 9) & 1);
  if (!(ctx->skip >> 2 & 1)) LDG_LAUNCH_ON(st, "linelocs", ldg_k_linelocs, n, 64, M_, ctx->video, ctx->vread, ctx->vchan, C, ctx->d_recs,
             ctx->d_peaks, ctx->d_lines, ctx->d_bad, ctx->d_sst, ctx->d_sbits);
  // per-line kernels: a read has at most linecount + 4 = frame_lines / 2 + 5 lines
  // (field.hip linelocs) and linecount <= frame_lines / 2 + 1 output rows, so the grids
  // stop there (MAX_LINES rows per read is PAL's bound: NTSC launched 53 - 57 empty
  // workgroups per read, each holding its LDS while it found its row out of range)
  const dim3 g_lines((unsigned)(C.frame_lines / 2 + 5), (unsigned)n), g_rows((unsigned)(C.frame_lines / 2 + 1), (unsigned)n);
  if (!(ctx->skip >> 3 & 1)) LDG_LAUNCH_ON(st, "hsync_lines", ldg_k_hsync_lines, g_lines, 64, M_, ctx->video, ctx->vread, ctx->vchan, C,
             ctx->d_recs, ctx->d_lines, ctx->d_bad, ctx->d_reads);
  if (!(ctx->skip >> 4 & 1)) LDG_LAUNCH_ON(st, "hsync_field", ldg_k_hsync_field, n, 256, M_, C, ctx->d_recs, ctx->d_lines, ctx->d_bad);
  if (!(ctx->skip >> 5 & 1)) LDG_LAUNCH_ON(st, "philips", ldg_k_philips, n, 192, M_, ctx->video, ctx->vread, ctx->vchan, C, ctx->d_recs,
             ctx->d_lines, ctx->d_reads);
  if (int rc = check_launch(ctx, "field kernels")) return rc;
  if (ctx->system == 0) {
    for (int pass = 0; pass < 2; pass++) {
      if (!(ctx->skip >> 6 & 1)) LDG_LAUNCH_ON(st, "burst_lines", ldg_k_burst_lines, g_lines, 64, M_, ctx->video, ctx->vread, ctx->vchan, C,
                 ctx->d_recs, ctx->d_lines, ctx->d_blevel, pass, ctx->d_bst, ctx->d_reads);
      if (!(ctx->skip >> 7 & 1)) LDG_LAUNCH_ON(st, "burst_field", ldg_k_burst_field, n, 64, M_, ctx->video, ctx->vread, ctx->vchan,
                 ctx->d_recs, ctx->d_lines, ctx->d_blevel, C, pass, ctx->d_bst, ctx->d_reads);
    }
  } else {
    LDG_LAUNCH_ON(st, "pilot_lines", ldg_k_pilot_lines, g_lines, 64, M_, ctx->video, ctx->vread, ctx->vchan, C,
               ctx->d_recs, ctx->d_lines, ctx->d_scratch, ctx->d_reads);
    LDG_LAUNCH_ON(st, "pilot_field", ldg_k_pilot_field, n, 256, M_, ctx->d_recs, ctx->d_lines, C, ctx->d_scratch,
               ctx->d_reads);
  }
  if (!(ctx->skip >> 8 & 1)) {
    if (C.hz_ire_r != 0.0)
      LDG_LAUNCH_ON(st, "final_lines", ldg_k_final_lines, g_rows, FINAL_NT, M_, ctx->video, ctx->vread, ctx->vchan, C,
                    ctx->d_recs, ctx->d_lines, ctx->d_blevel, ctx->d_pic, ctx->pic_stride, ctx->d_reads);
    else
      LDG_LAUNCH_ON(st, "final_lines", ldg_k_final_lines_div, g_rows, FINAL_NT, M_, ctx->video, ctx->vread, ctx->vchan, C,
                    ctx->d_recs, ctx->d_lines, ctx->d_blevel, ctx->d_pic, ctx->pic_stride, ctx->d_reads);
  }
  // (pending records become FS_VALID in ldg_k_recs_out, after all groups)
  if (int rc = check_launch(ctx, "tbc kernels")) return rc;
  return LDG_OK;
}

// LDG_HOSTPROF=1: host time spent between points of ldg_decode_reads_async (stderr)
struct HostProf {
  bool on = getenv("LDG_HOSTPROF") != nullptr;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), t = t0;
  char buf[512];
  int len = 0;
  void mark(const char* what) {
    if (!on) return;
    const auto u = std::chrono::steady_clock::now();
    len += snprintf(buf + len, sizeof(buf) - len > 0 ? sizeof(buf) - len : 0, " %s %.0f",
                    what, std::chrono::duration<double, std::micro>(u - t).count());
    t = u;
  }
  ~HostProf() {
    if (on) fprintf(stderr, "[hostprof] total %.0f us:%s\n",
                    std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), buf);
  }
};

int ldg_decode_reads_async(ldg_ctx* ctx, int n, const int64_t* read_starts, const double* mtf,
                           const int32_t* slots) {
  return ldg_decode_reads_async2(ctx, n, read_starts, mtf, slots, nullptr);
}

int ldg_set_video_cut(ldg_ctx* ctx, int64_t out_samples) {
  if (!ctx || out_samples < 0) return LDG_EINVAL;
  ctx->video_cut = out_samples;
  return LDG_OK;
}

// A read's overlap-save geometry from its start (lddecode_core.py:373-385; the
// probe pick kernel moves a read with the same formulas).
static void read_geometry(ReadDesc& r, int64_t start) {
  r.readsample = start;
  r.end = start + READLEN + 1;
  r.s0 = start > BLOCKCUT ? start - BLOCKCUT : 0;
  r.n_out = (int32_t)(r.end - r.s0 + 1);
  r.n_blocks = (int32_t)((r.end - r.s0 + BLOCKSTEP - 1) / BLOCKSTEP);
  r.n_audio = (int32_t)((r.end - r.s0) / AUDIO_DIV1 + 1);
  r.n_audio2 = r.n_audio / AUDIO_DIV2;
  const TailPlan tp = tail_plan(r.n_audio, r.n_audio2, r.vcut);   // r.vcut is set before the geometry
  r.acut1 = tp.acut1;
  r.acut2 = tp.acut2;
}

// The tail plan of a read of this geometry under the video cut vcut (tail.hpp), for tests:
// out = {acut1, acut2, live audio phase-2 blocks, demod blocks that make audio slices,
// demod blocks that store demod_05}; -1 for "no cut".  Needs no context and no GPU.
int ldg_tail_plan(int64_t n_out, int64_t n_audio, int64_t n_audio2, int64_t vcut, int64_t out[5]) {
  if (!out || n_out < 0 || n_out > MAX_NOUT || n_audio < 0 || n_audio > MAX_NAUDIO || n_audio2 < 0 ||
      n_audio2 > MAX_NAUDIO2 || vcut < 0)
    return LDG_EINVAL;
  const TailPlan tp = tail_plan((int)n_audio, (int)n_audio2, vcut > 0 ? vcut : INT64_MAX);
  const int n_blocks = (int)((n_out - 1 + BLOCKSTEP - 1) / BLOCKSTEP), n_mid = a2_n_mid((int)n_audio);
  out[0] = tp.acut1 == ACUT_NONE ? -1 : tp.acut1;
  out[1] = tp.acut2 == ACUT_NONE ? -1 : tp.acut2;
  out[2] = out[3] = out[4] = 0;
  for (int j = 0; j <= n_mid + 1; j++) out[2] += !a2_block_dead(j, n_mid, tp.acut2);
  for (int b = 0; b < n_blocks; b++) {
    out[3] += !a1_block_dead(b, tp.acut1);
    out[4] += !(vcut > 0 && (int64_t)b * BLOCKSTEP >= vcut);
  }
  return LDG_OK;
}

// divconst.hpp's division by a constant over n operands, for tests: out[i] = div_const
// (guarded != 0) or div_const_nz of x[i] with c and RN(1 / c), the sequence the row kernels
// run.  LDG_EINVAL when c fails divconst_ok (x or out null: only that check is made).
// Needs no context and no GPU.
int ldg_div_const(const double* x, int64_t n, double c, int guarded, double* out) {
  if (!divconst_ok(c) || n < 0) return LDG_EINVAL;
  if (!x || !out) return LDG_OK;
  const double r = 1.0 / c;
  for (int64_t i = 0; i < n; i++) out[i] = guarded ? div_const(x[i], c, r) : div_const_nz(x[i], c, r);
  return LDG_OK;
}

// The span of sample positions ldg_k_audio_ds can form from a field's final line
// locations (tail.hpp; the device guard flags FS_VCUT unless it lies in [0, 64 acut2)):
// out = {lowest position, highest position}.  Needs no context and no GPU.
int ldg_audio_reach(const double* lines, int nlines, int linecount, double linelen, double out[2]) {
  if (!lines || !out || nlines <= 0 || nlines > MAX_LINES || linecount < 0) return LDG_EINVAL;
  double lo = __builtin_inf(), hi = -__builtin_inf();
  for (int il = 0; il <= audio_last_line(nlines, linecount); il++) {
    double a, b;
    audio_line_span(lines, nlines, il, linelen, a, b);
    if (!(a == a)) { lo = hi = a; break; }
    lo = std::min(lo, a);
    hi = std::max(hi, b);
  }
  out[0] = lo;
  out[1] = hi;
  return LDG_OK;
}

// ldg_k_probe_pick's half-window: it moves a probed read by at most this many samples
// (0.3 lines; GPUDecoder.probe_win is the same figure)
static int probe_halfwin(const SysConst& C) { return (int)(3 * (int64_t)C.linelen / 10); }

int ldg_decode_reads_async2(ldg_ctx* ctx, int n, const int64_t* read_starts, const double* mtf,
                            const int32_t* slots, uint8_t* full) {
  if (!ctx || n <= 0 || n > ctx->max_reads || !read_starts || !mtf) return LDG_EINVAL;
  if (ctx->ncalls >= ldg_ctx::MAX_CALLS) {
    ctx->err = "too many decodes outstanding";
    return LDG_ESTATE;
  }
  if (!ctx->have_filters || !ctx->cap) {
    ctx->err = "filters or capture not set";
    return LDG_ESTATE;
  }
  LDG_TRY(hipSetDevice(ctx->device));
  if (const char* e = getenv("LDG_STAGES")) ctx->stages = atoi(e);   // stage-isolation probes only
  if (const char* e = getenv("LDG_SKIP")) ctx->skip = atoi(e);       // timing probes only: results are garbage
  HostProf hp_;
  // consecutive calls' demods alternate between two streams: the next call's demod
  // workgroups take CUs as the current one's last wave drains (its tail, and the
  // field chains' gaps), instead of queueing behind it.  Every consumer waits on
  // the call's ev_demod, and two demod workgroups never share a CU (LDS), so the
  // per-CU park stays private.
  hipStream_t s = (ctx->demod_streams == 2 && (ctx->seq & 1)) ? ctx->stream_b : ctx->stream;
  const int R = ctx->max_reads;
  std::vector<int32_t> smap(n);
  std::vector<char> used(R, 0);
  for (int q = 0; q < ctx->ncalls; q++)          // slots of outstanding calls are busy
    for (int32_t sl : ctx->calls[(ctx->call_head + q) % ldg_ctx::MAX_CALLS].smap) used[sl] = 1;
  for (int i = 0; i < n; i++) {
    smap[i] = slots ? slots[i] : i;
    if (smap[i] < 0 || smap[i] >= R || used[smap[i]]) {
      ctx->err = "bad, duplicate or busy slot";
      return LDG_EINVAL;
    }
    used[smap[i]] = 1;
  }
  ctx->h_reads.resize(R);
  std::vector<ReadDesc> nr(n);
  std::map<double, int> mtf_slot;
  std::vector<double> tm;
  for (int i = 0; i < n; i++) {
    ReadDesc r{};
    const int64_t start = read_starts[i];
    r.vcut = (ctx->video_cut > 0 && !(full && (full[i] & LDG_READ_FULL))) ? ctx->video_cut : INT64_MAX;
    read_geometry(r, start);
    if (r.n_out > MAX_NOUT || r.n_blocks > MAX_BLOCKS_PER_READ) {
      ctx->err = "read geometry out of range";
      return LDG_EINVAL;
    }
    auto it = mtf_slot.find(mtf[i]);
    if (it == mtf_slot.end()) {
      r.filt_slot = mtf_slot[mtf[i]] = (int)tm.size();
      tm.push_back(mtf[i]);
    } else {
      r.filt_slot = it->second;
    }
    nr[i] = r;
  }
  const int ci = (ctx->call_head + ctx->ncalls) % ldg_ctx::MAX_CALLS;
  ldg_ctx::Call& call = ctx->calls[ci];
  int32_t* dsm = ctx->d_smap + (size_t)ci * R;
  // read setup on sprep, reading the pinned parameter block in place (no copy
  // packets): this call's slots are not busy, and its rf tables (one set per
  // call index) were last read by the demod of the call two back
  char* hp = ctx->h_prep + (size_t)ci * ctx->prep_bytes;
  ReadDesc* hnr = (ReadDesc*)hp;
  int32_t* hsm = (int32_t*)(hp + (size_t)R * sizeof(ReadDesc));
  double* htm = (double*)(hp + (size_t)R * (sizeof(ReadDesc) + sizeof(int32_t)));
  std::memcpy(hnr, nr.data(), n * sizeof(ReadDesc));
  std::memcpy(hsm, smap.data(), n * sizeof(int32_t));
  std::memcpy(htm, tm.data(), tm.size() * sizeof(double));
  if (ctx->rf_cap[ci] < (int)tm.size()) {
    // grow this call index's tables: the last demod that read them must be done
    if (call.demod_recorded) LDG_TRY(hipEventSynchronize(call.ev_demod));
    const int want = std::min(R, std::max((int)tm.size(), std::max(8, 2 * ctx->rf_cap[ci])));
    dfree(ctx->rf_tab[ci]);
    ctx->rf_tab[ci] = nullptr;
    ctx->rf_cap[ci] = 0;
    if (int rc = dmalloc(ctx, &ctx->rf_tab[ci], (size_t)want * BLOCKLEN)) return rc;
    ctx->rf_cap[ci] = want;
  }
  ctx->rf_cur = ctx->rf_tab[ci];
  if (ctx->cs && (ctx->stages & 1)) {
    // a streamed capture: the samples this call's blocks (and start probes) read are in
    // the ring before its demod runs, and the kernels get the window they may read.
    // A read flagged LDG_READ_PROBE may be moved by ldg_k_probe_pick by up to the probe's
    // half-window either way, and is flagged before it is known whether its probe runs:
    // the window's high end covers every flagged read's last block at the far end of that
    // range (a window cut at the predicted start's last block gave the moved read's last
    // block FS_EOF).  Its low end is the released point, which the host keeps STREAM_MARGIN
    // below the replay (ldgpu/decoder.py): that covers a read moved back and its probe.
    int64_t hi = 0;
    for (int i = 0; i < n; i++) {
      const int64_t w = (full && (full[i] & LDG_READ_PROBE)) ? probe_halfwin(ctx->C) : 0;
      hi = std::max(hi, nr[i].s0 + (int64_t)(nr[i].n_blocks - 1) * BLOCKSTEP + BLOCKLEN + w);
    }
    if (int rc = stream_prepare(ctx, s, hi)) return rc;
  }
  // start probes: the one block centred on each flagged read's (predicted) start,
  // where it lies inside the capture
  ReadDesc* hpr = (ReadDesc*)(ctx->h_probe + (size_t)ci * R * (sizeof(ReadDesc) + sizeof(int32_t)));
  int32_t* hps = (int32_t*)(hpr + R);
  int np = 0;
  if (full)
    for (int i = 0; i < n; i++) {
      if (!(full[i] & LDG_READ_PROBE)) continue;
      ReadDesc pr = nr[i];
      const int64_t r0 = nr[i].readsample - PROBE_C;
      if (!(ctx->stages & 1) || r0 - BLOCKCUT < ctx->cap_first ||
          r0 - BLOCKCUT + BLOCKLEN > ctx->cap_first + ctx->cap_nsamp) {
        full[i] &= (uint8_t)~LDG_READ_PROBE;      // not probed: the caller learns it from the flag
        continue;
      }
      read_geometry(pr, r0);
      pr.end = r0 + BLOCKSTEP + 64;               // one block (output [0, BLOCKSTEP))
      pr.n_out = (int32_t)(pr.end - pr.s0 + 1);
      pr.n_blocks = 1;
      pr.n_audio = (int32_t)((pr.end - pr.s0) / AUDIO_DIV1 + 1);
      pr.n_audio2 = pr.n_audio / AUDIO_DIV2;
      pr.vcut = 0;                                // the demod stops after the sync channel
      pr.acut1 = pr.acut2 = ACUT_NONE;
      hpr[np] = pr;
      hps[np++] = smap[i];
    }
  int32_t* dps = ctx->d_psm + (size_t)ci * R;
  hipStream_t sp = ctx->sprep;
  if (call.demod_recorded) LDG_TRY(hipStreamWaitEvent(sp, call.ev_demod, 0));
  LDG_LAUNCH_ON(sp, "new_reads", ldg_k_new_reads, (n + 255) / 256, 256, hnr, hsm, n, dsm, ctx->d_reads, ctx->d_status);
  if (np) LDG_LAUNCH_ON(sp, "new_reads", ldg_k_new_reads, (np + 255) / 256, 256, hpr, hps, np, dps, ctx->d_preads,
                        ctx->d_status);
    LDG_LAUNCH_ON(sp, "rf_table", ldg_k_rf_table, dim3(BLOCKLEN / 256, (unsigned)tm.size()), 256, ctx->rfvideo, ctx->mtf,
                  ctx->mtf_logabs, ctx->mtf_arg, htm, ctx->rf_cur);
  if (int rc = check_launch(ctx, "ldg_k_rf_table")) return rc;
  LDG_TRY(hipEventRecord(call.ev_prep, sp));
  LDG_TRY(hipStreamWaitEvent(s, call.ev_prep, 0));
  // with concealment the last frame assembly also read its slots' demod channel
  // (ldg_k_dropout_lines), which this call's demod rewrites in the slots it reuses
  if (ctx->frames_recorded && ctx->frames_demod) LDG_TRY(hipStreamWaitEvent(s, ctx->ev_frames, 0));
  hp_.mark("prep");
  if (np && (ctx->stages & 1)) {
    // the probes, then the reads they move, on the demod stream ahead of the demod
    const SysConst C = ctx->C;
    LDG_LAUNCH_ON(s, "demod_probe", ldg_k_demod_probe, np, 1024, dps, ctx->d_preads, ctx->cap, ctx->cap_first,
                  ctx->cap_nsamp, ctx->cap_ring, ctx->fmt, ctx->tw, ctx->twk, ctx->rf_cur, ctx->fvideo, ctx->f05, ctx->iirtab,
                  ctx->alf, ctx->arf, C, ctx->video, ctx->vread, ctx->vchan,
                  ctx->d_status, ctx->d_ospill, ++ctx->park_epoch, ctx->d_stile, ctx->d_aslice, ctx->d_sst,
                  ctx->d_sbits, ctx->d_bst, nullptr);
    LDG_LAUNCH_ON(s, "probe_pick", ldg_k_probe_pick, np, 64, dps, ctx->d_preads, ctx->d_reads, ctx->d_status,
                  ctx->d_sst, ctx->d_sbits, C, probe_halfwin(C));
    if (int rc = check_launch(ctx, "ldg_k_probe_pick")) return rc;
    ctx->probes += np;
  }
  // field-chain groups: consecutive reads, one group per sub-stream
  const int ng = (ctx->stages & 4) ? std::max(1, std::min(ctx->nsub, n / 4)) : 0;
  auto group = [&](int g, int& i0, int& m) {
    i0 = (int)((int64_t)n * g / ng);
    m = (int)((int64_t)n * (g + 1) / ng) - i0;
  };
  if (ctx->stages & 1)
    if (int rc = launch_demod(ctx, s, n, dsm)) return rc;
  hp_.mark("demod");
  LDG_TRY(hipEventRecord(call.ev_demod, s));
  call.demod_recorded = true;
  // audio phases 1 and 2 on their own stream; they rewrite the slots' audio, which
  // an outstanding ldg_field_audio_async may still be reading
  LDG_TRY(hipStreamWaitEvent(ctx->sa, call.ev_demod, 0));
  if (ctx->audio_recorded) LDG_TRY(hipStreamWaitEvent(ctx->sa, ctx->ev_audio, 0));
  if (ctx->stages & 2) LDG_LAUNCH_ON(ctx->sa, "audio1", ldg_k_audio1, n * MAX_BLOCKS_PER_READ, A1_T, dsm, ctx->d_reads,
                                     ctx->tw, ctx->C, ctx->d_aslice, ctx->audio1, ctx->a1read, ctx->a1chan, ctx->d_status);
  if (ctx->stages & 2) LDG_LAUNCH_ON(ctx->sa, "audio2", ldg_k_audio2, n * AUDIO2_WG, 1024, dsm, ctx->d_reads, ctx->tw, ctx->lpf2, ctx->audio1,
                ctx->a1read, ctx->a1chan, ctx->audio2, ctx->a2read, ctx->a2chan, ctx->d_status);
  if (int rc = check_launch(ctx, "ldg_k_audio2")) return rc;
  LDG_TRY(hipEventRecord(call.ev_done[0], ctx->sa));
  hp_.mark("audio");
  // field chains: they rewrite the slots' records and pictures, so they also
  // wait for the last frame assembly
  int nd = 1;
  for (int g = 0; g < ng; g++) {
    int i0, m;
    group(g, i0, m);
    if (m <= 0) continue;
    hipStream_t st = ctx->sub[g];
    LDG_TRY(hipStreamWaitEvent(st, call.ev_demod, 0));
    if (ctx->frames_recorded) LDG_TRY(hipStreamWaitEvent(st, ctx->ev_frames, 0));
    if (ctx->audio_recorded) LDG_TRY(hipStreamWaitEvent(st, ctx->ev_audio, 0));
    if (int rc = launch_chain(ctx, st, m, dsm + i0)) return rc;
    LDG_TRY(hipEventRecord(call.ev_done[nd++], st));
  hp_.mark("chain");
  }
  call.ndone = nd;
  // the records to pinned host memory as soon as the call's chains are done
  for (int k = 0; k < nd; k++) LDG_TRY(hipStreamWaitEvent(ctx->srec, call.ev_done[k], 0));
  call.seq = ++ctx->seq;
  LDG_LAUNCH_ON(ctx->srec, "recs_out", ldg_k_recs_out, 1, 256, ctx->d_recs, dsm, n, ctx->d_reads,
                ctx->h_recs_pin + (size_t)ci * R,
                ctx->h_done + ci, call.seq);
  LDG_TRY(hipEventRecord(call.ev_copied, ctx->srec));
  hp_.mark("rec");
  call.n = n;
  call.smap = smap;
  for (int i = 0; i < n; i++) {
    ctx->h_reads[smap[i]] = nr[i];
    ctx->live[smap[i]] = 0;        // not readable until the wait
  }
  ctx->ncalls++;
  return LDG_OK;
}

int ldg_decode_reads_wait(ldg_ctx* ctx, ldg_field_info* info) {
  if (!ctx || !info) return LDG_EINVAL;
  if (!ctx->ncalls) {
    ctx->err = "no decode outstanding";
    return LDG_ESTATE;
  }
  LDG_TRY(hipSetDevice(ctx->device));
  ldg_ctx::Call& call = ctx->calls[ctx->call_head];
  // the records of this call's slots are final (other slots may have been in flight):
  // poll the completion word, checking the event now and then for errors
  for (uint32_t it = 1;; it++) {
    if (__atomic_load_n(ctx->h_done + ctx->call_head, __ATOMIC_ACQUIRE) == call.seq) break;
    if ((it & 255) == 0) {
      const hipError_t q = hipEventQuery(call.ev_copied);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) LDG_TRY(q);
      if (it > 4096) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    __builtin_ia32_pause();
  }
  prof_collect(ctx);
  const FieldRec* recs = ctx->h_recs_pin + (size_t)ctx->call_head * ctx->max_reads;
  for (int i = 0; i < call.n; i++) {
    info[i] = recs[i];
    ctx->live[call.smap[i]] = 1;
    ReadDesc& hr = ctx->h_reads[call.smap[i]];
    if (recs[i].readsample != hr.readsample) read_geometry(hr, recs[i].readsample);   // moved by its probe
  }
  call.smap.clear();
  call.n = 0;
  ctx->call_head = (ctx->call_head + 1) % ldg_ctx::MAX_CALLS;
  ctx->ncalls--;
  return LDG_OK;
}

int ldg_decode_reads(ldg_ctx* ctx, int n, const int64_t* read_starts, const double* mtf, const int32_t* slots,
                     ldg_field_info* info) {
  if (!info) return LDG_EINVAL;
  if (int rc = ldg_decode_reads_async(ctx, n, read_starts, mtf, slots)) return rc;
  return ldg_decode_reads_wait(ctx, info);
}

// The 48 kHz audio outputs of n fields: device -> the context's pinned buffers
// on stream s, wait, then into the caller's arrays (counts[i] = -1 where the
// reference raises).
static int audio_out(ldg_ctx* ctx, hipStream_t s, int n, int16_t* pcm, int64_t pcm_stride, int32_t* counts,
                     double* next_offsets) {
  LDG_TRY(hipMemcpyAsync(ctx->h_pcm, ctx->d_pcm, (size_t)n * PCM_STRIDE * sizeof(int16_t), hipMemcpyDeviceToHost, s));
  LDG_TRY(hipMemcpyAsync(ctx->h_counts, ctx->d_counts, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LDG_TRY(hipMemcpyAsync(ctx->h_next, ctx->d_next, n * sizeof(double), hipMemcpyDeviceToHost, s));
  LDG_TRY(hipMemcpyAsync(ctx->h_aerr, ctx->d_aerr, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LDG_TRY(hipStreamSynchronize(s));
  prof_collect(ctx);
  size_t at = 0;                  // pcm_stride 0: packed, field after field
  for (int i = 0; i < n; i++) {
    counts[i] = ctx->h_aerr[i] ? -1 : ctx->h_counts[i];
    next_offsets[i] = ctx->h_next[i];
    const int c = ctx->h_counts[i] > 0 ? ctx->h_counts[i] : 0;
    const size_t len = (size_t)(2 * c < PCM_STRIDE ? 2 * c : PCM_STRIDE);
    std::memcpy(pcm + (pcm_stride ? (size_t)i * pcm_stride : at), ctx->h_pcm + (size_t)i * PCM_STRIDE,
                len * sizeof(int16_t));
    at += len;
  }
  return LDG_OK;
}

// ldg_field_audio in two halves: launch (the outputs land in the context's
// pinned buffers, an event marks them), then collect.  One outstanding.
int ldg_field_audio_async(ldg_ctx* ctx, int n, const int32_t* slots, const double* offsets) {
  if (!ctx || n < 0 || n > ctx->max_reads || (n && (!slots || !offsets))) return LDG_EINVAL;
  if (ctx->audio_pending >= 0) {
    ctx->err = "an audio launch is already outstanding";
    return LDG_ESTATE;
  }
  for (int i = 0; i < n; i++)
    if (slots[i] < 0 || slots[i] >= ctx->max_reads || !ctx->live[slots[i]]) return LDG_EINVAL;
  LDG_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->sout;
  if (n) {
    ctx->h_idx.assign(slots, slots + n);
    if (int rc = stage_h2d(ctx, ctx->d_idx, ctx->h_idx.data(), n * sizeof(int64_t), s)) return rc;
    if (int rc = stage_h2d(ctx, ctx->d_offsets, offsets, n * sizeof(double), s)) return rc;
    LDG_TRY(hipMemsetAsync(ctx->d_aerr, 0, n * sizeof(int32_t), s));
    LDG_LAUNCH_ON(s, "audio_ds", ldg_k_audio_ds, n, 256, ctx->d_idx, ctx->d_offsets, ctx->d_recs,
               ctx->d_lines + LLF * MAX_LINES, (int64_t)LINES_STRIDE, ctx->audio2, ctx->a2read, ctx->a2chan, ctx->C,
               ctx->d_pcm, PCM_STRIDE, ctx->d_counts, ctx->d_next, ctx->d_aerr);
    if (int rc = check_launch(ctx, "ldg_k_audio_ds")) return rc;
    LDG_TRY(hipMemcpyAsync(ctx->h_pcm, ctx->d_pcm, (size_t)n * PCM_STRIDE * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    LDG_TRY(hipMemcpyAsync(ctx->h_counts, ctx->d_counts, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    LDG_TRY(hipMemcpyAsync(ctx->h_next, ctx->d_next, n * sizeof(double), hipMemcpyDeviceToHost, s));
    LDG_TRY(hipMemcpyAsync(ctx->h_aerr, ctx->d_aerr, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  }
  LDG_TRY(hipEventRecord(ctx->ev_audio, s));
  ctx->audio_recorded = true;
  ctx->audio_pending = n;
  return LDG_OK;
}

int ldg_field_audio_collect(ldg_ctx* ctx, int16_t* pcm, int64_t pcm_stride, int32_t* counts, double* next_offsets) {
  if (!ctx) return LDG_EINVAL;
  if (ctx->audio_pending < 0) {
    ctx->err = "no audio launch outstanding";
    return LDG_ESTATE;
  }
  const int n = ctx->audio_pending;
  if (n && (!pcm || !counts || !next_offsets || pcm_stride < PCM_STRIDE)) return LDG_EINVAL;
  LDG_TRY(hipEventSynchronize(ctx->ev_audio));
  ctx->audio_pending = -1;
  for (int i = 0; i < n; i++) {
    counts[i] = ctx->h_aerr[i] ? -1 : ctx->h_counts[i];
    next_offsets[i] = ctx->h_next[i];
    const int c = ctx->h_counts[i] > 0 ? ctx->h_counts[i] : 0;
    std::memcpy(pcm + (size_t)i * pcm_stride, ctx->h_pcm + (size_t)i * PCM_STRIDE,
                (size_t)(2 * c < PCM_STRIDE ? 2 * c : PCM_STRIDE) * sizeof(int16_t));
  }
  return LDG_OK;
}

int ldg_field_audio(ldg_ctx* ctx, int n, const int32_t* slots, const double* offsets, int16_t* pcm,
                    int64_t pcm_stride, int32_t* counts, double* next_offsets) {
  if (!ctx || n < 0 || n > ctx->max_reads || (n && (!slots || !offsets || !pcm || !counts || !next_offsets)))
    return LDG_EINVAL;
  if (n == 0) return LDG_OK;
  if (pcm_stride < PCM_STRIDE) return LDG_EINVAL;
  for (int i = 0; i < n; i++)
    if (slots[i] < 0 || slots[i] >= ctx->max_reads || !ctx->live[slots[i]]) return LDG_EINVAL;
  LDG_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->sout;     // output work: overlaps the outstanding decodes
  ctx->h_idx.assign(slots, slots + n);
  if (int rc = stage_h2d(ctx, ctx->d_idx, ctx->h_idx.data(), n * sizeof(int64_t), s)) return rc;
  if (int rc = stage_h2d(ctx, ctx->d_offsets, offsets, n * sizeof(double), s)) return rc;
  LDG_TRY(hipMemsetAsync(ctx->d_aerr, 0, n * sizeof(int32_t), s));
  LDG_LAUNCH_ON(s, "audio_ds", ldg_k_audio_ds, n, 256, ctx->d_idx, ctx->d_offsets, ctx->d_recs,
             ctx->d_lines + LLF * MAX_LINES, (int64_t)LINES_STRIDE, ctx->audio2, ctx->a2read, ctx->a2chan, ctx->C,
             ctx->d_pcm, PCM_STRIDE, ctx->d_counts, ctx->d_next, ctx->d_aerr);
  if (int rc = check_launch(ctx, "ldg_k_audio_ds")) return rc;
  return audio_out(ctx, s, n, pcm, pcm_stride, counts, next_offsets);
}

// ---- field archive --------------------------------------------------------------
static int archive_reserve(ldg_ctx* ctx, int64_t need) {
  if (need <= ctx->arch_cap) return LDG_OK;
  int64_t cap = ctx->arch_cap ? ctx->arch_cap : 1024;
  while (cap < need) cap *= 2;
  FieldRec* r = nullptr;
  double *l = nullptr, *a = nullptr;
  if (dmalloc(ctx, &r, (size_t)cap) || dmalloc(ctx, &l, (size_t)cap * MAX_LINES) ||
      dmalloc(ctx, &a, (size_t)cap * ctx->a2read)) {
    dfree(r); dfree(l); dfree(a);
    return LDG_ENOMEM;
  }
  hipStream_t s = ctx->sout;     // output work: overlaps the outstanding decodes
  if (ctx->arch_cap) {
    LDG_TRY(hipMemcpyAsync(r, ctx->arch_recs, ctx->arch_cap * sizeof(FieldRec), hipMemcpyDeviceToDevice, s));
    LDG_TRY(hipMemcpyAsync(l, ctx->arch_lines, ctx->arch_cap * MAX_LINES * sizeof(double), hipMemcpyDeviceToDevice, s));
    LDG_TRY(hipMemcpyAsync(a, ctx->arch_audio2, ctx->arch_cap * ctx->a2read * sizeof(double),
                           hipMemcpyDeviceToDevice, s));
    LDG_TRY(hipStreamSynchronize(s));
    dfree(ctx->arch_recs); dfree(ctx->arch_lines); dfree(ctx->arch_audio2);
  }
  ctx->arch_recs = r; ctx->arch_lines = l; ctx->arch_audio2 = a;
  ctx->arch_cap = cap;
  return LDG_OK;
}

int ldg_audio_offsets(double o0, int64_t n, const double* linecounts, double line_period, double* out) {
  if (n < 0 || (n && !linecounts) || !out) return LDG_EINVAL;
  const double gap = 1 / 48000.0;
  double o = o0;
  out[0] = o;
  for (int64_t k = 0; k < n; k++) {
    const double frametime = (line_period * linecounts[k]) / 1000000;
    const double c = std::ceil(((frametime + gap) - o) / gap);   // numpy: ceil((stop - start) / step)
    if (!(c >= 1)) return LDG_EINVAL;
    double last;
    if (c == 1) last = o;
    else if (c == 2) last = o + gap;
    else last = o + (c - 1) * ((o + gap) - o);                       // DOUBLE_fill: start + i * delta
    o = last - frametime;
    out[k + 1] = o;
  }
  return LDG_OK;
}

int ldg_archive_fields(ldg_ctx* ctx, int n, const int32_t* slots, int64_t first) {
  if (!ctx || n < 0 || n > ctx->max_reads || first < 0 || (n && !slots)) return LDG_EINVAL;
  for (int i = 0; i < n; i++)
    if (slots[i] < 0 || slots[i] >= ctx->max_reads || !ctx->live[slots[i]]) return LDG_EINVAL;
  if (n == 0) return LDG_OK;
  LDG_TRY(hipSetDevice(ctx->device));
  if (int rc = archive_reserve(ctx, first + n)) return rc;
  hipStream_t s = ctx->sout;     // output work: overlaps the outstanding decodes
  // one gather launch on the output stream, no host wait: the slots' next writers
  // (audio phase 2 on sa, the field chains) wait for ev_audio, recorded behind it
  ctx->h_idx.assign(slots, slots + n);
  if (int rc = stage_h2d(ctx, ctx->d_idx, ctx->h_idx.data(), n * sizeof(int64_t), s)) return rc;
  const int chunks = (int)std::min<int64_t>(64, (std::max<int64_t>(ctx->a2read, MAX_LINES) + 1023) / 1024);
  LDG_LAUNCH_ON(s, "archive", ldg_k_archive, dim3(chunks, n), 256, ctx->d_idx, first, ctx->d_recs, ctx->d_lines,
                ctx->audio2, ctx->a2read, ctx->arch_recs, ctx->arch_lines, ctx->arch_audio2);
  if (int rc = check_launch(ctx, "ldg_k_archive")) return rc;
  LDG_TRY(hipEventRecord(ctx->ev_audio, s));
  ctx->audio_recorded = true;
  return LDG_OK;
}

static void arch_audio_free(ldg_ctx* ctx) {
  auto& a = ctx->aa;
  for (void* p : {(void*)a.d_idx, (void*)a.d_off, (void*)a.d_pcm, (void*)a.d_counts, (void*)a.d_next, (void*)a.d_err})
    if (p) (void)hipFree(p);
  if (a.h) (void)hipHostFree(a.h);
  a = ldg_ctx::ArchAudio{};
}

// n entries > max_reads: one launch and one copy back for all of them
static int arch_audio_big(ldg_ctx* ctx, int n, const int64_t* entries, const double* offsets, int16_t* pcm,
                          int64_t pcm_stride, int32_t* counts, double* next_offsets) {
  auto& a = ctx->aa;
  if (n > a.cap) {
    arch_audio_free(ctx);
    const int64_t cap = (std::max<int64_t>(n, 4096) + 7) & ~(int64_t)7;   // keeps the pinned arrays 8-byte aligned
    const size_t hb = (size_t)cap * (sizeof(int64_t) + sizeof(double) + PCM_STRIDE * sizeof(int16_t) +
                                     sizeof(int32_t) + sizeof(double) + sizeof(int32_t));
    if (hipMalloc(&a.d_idx, cap * sizeof(int64_t)) != hipSuccess || hipMalloc(&a.d_off, cap * sizeof(double)) != hipSuccess ||
        hipMalloc(&a.d_pcm, (size_t)cap * PCM_STRIDE * sizeof(int16_t)) != hipSuccess ||
        hipMalloc(&a.d_counts, cap * sizeof(int32_t)) != hipSuccess || hipMalloc(&a.d_next, cap * sizeof(double)) != hipSuccess ||
        hipMalloc(&a.d_err, cap * sizeof(int32_t)) != hipSuccess || hipHostMalloc((void**)&a.h, hb, hipHostMallocDefault) != hipSuccess) {
      arch_audio_free(ctx);
      return LDG_ENOMEM;
    }
    a.cap = cap;
  }
  int64_t* h_idx = (int64_t*)a.h;
  double* h_off = (double*)(h_idx + a.cap);
  int16_t* h_pcm = (int16_t*)(h_off + a.cap);
  int32_t* h_counts = (int32_t*)(h_pcm + (size_t)a.cap * PCM_STRIDE);
  double* h_next = (double*)(h_counts + a.cap);
  int32_t* h_err = (int32_t*)(h_next + a.cap);
  std::memcpy(h_idx, entries, n * sizeof(int64_t));
  std::memcpy(h_off, offsets, n * sizeof(double));
  hipStream_t s = ctx->sout;
  LDG_TRY(hipMemcpyAsync(a.d_idx, h_idx, n * sizeof(int64_t), hipMemcpyHostToDevice, s));
  LDG_TRY(hipMemcpyAsync(a.d_off, h_off, n * sizeof(double), hipMemcpyHostToDevice, s));
  LDG_TRY(hipMemsetAsync(a.d_err, 0, n * sizeof(int32_t), s));
  LDG_LAUNCH_ON(s, "audio_ds", ldg_k_audio_ds, n, 256, a.d_idx, a.d_off, ctx->arch_recs, ctx->arch_lines,
                (int64_t)MAX_LINES, ctx->arch_audio2, ctx->a2read, ctx->a2chan, ctx->C, a.d_pcm, PCM_STRIDE,
                a.d_counts, a.d_next, a.d_err);
  if (int rc = check_launch(ctx, "ldg_k_audio_ds")) return rc;
  LDG_TRY(hipMemcpyAsync(h_pcm, a.d_pcm, (size_t)n * PCM_STRIDE * sizeof(int16_t), hipMemcpyDeviceToHost, s));
  LDG_TRY(hipMemcpyAsync(h_counts, a.d_counts, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LDG_TRY(hipMemcpyAsync(h_next, a.d_next, n * sizeof(double), hipMemcpyDeviceToHost, s));
  LDG_TRY(hipMemcpyAsync(h_err, a.d_err, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LDG_TRY(hipStreamSynchronize(s));
  prof_collect(ctx);
  size_t at = 0;                  // pcm_stride 0: packed, field after field
  for (int i = 0; i < n; i++) {
    counts[i] = h_err[i] ? -1 : h_counts[i];
    next_offsets[i] = h_next[i];
    const int c = h_counts[i] > 0 ? h_counts[i] : 0;
    const size_t len = (size_t)(2 * c < PCM_STRIDE ? 2 * c : PCM_STRIDE);
    std::memcpy(pcm + (pcm_stride ? (size_t)i * pcm_stride : at), h_pcm + (size_t)i * PCM_STRIDE, len * sizeof(int16_t));
    at += len;
  }
  return LDG_OK;
}

int ldg_archive_audio(ldg_ctx* ctx, int n, const int64_t* entries, const double* offsets, int16_t* pcm,
                      int64_t pcm_stride, int32_t* counts, double* next_offsets) {
  if (!ctx || n < 0 || (n && (!entries || !offsets || !pcm || !counts || !next_offsets))) return LDG_EINVAL;
  if (n == 0) return LDG_OK;
  if (pcm_stride != 0 && pcm_stride < PCM_STRIDE) return LDG_EINVAL;
  for (int i = 0; i < n; i++)
    if (entries[i] < 0 || entries[i] >= ctx->arch_cap) return LDG_EINVAL;
  LDG_TRY(hipSetDevice(ctx->device));
  if (n > ctx->max_reads) return arch_audio_big(ctx, n, entries, offsets, pcm, pcm_stride, counts, next_offsets);
  hipStream_t s = ctx->sout;     // output work: overlaps the outstanding decodes
  if (int rc = stage_h2d(ctx, ctx->d_idx, entries, n * sizeof(int64_t), s)) return rc;
  if (int rc = stage_h2d(ctx, ctx->d_offsets, offsets, n * sizeof(double), s)) return rc;
  LDG_TRY(hipMemsetAsync(ctx->d_aerr, 0, n * sizeof(int32_t), s));
  LDG_LAUNCH_ON(s, "audio_ds", ldg_k_audio_ds, n, 256, ctx->d_idx, ctx->d_offsets, ctx->arch_recs, ctx->arch_lines,
             (int64_t)MAX_LINES, ctx->arch_audio2, ctx->a2read, ctx->a2chan, ctx->C, ctx->d_pcm, PCM_STRIDE,
             ctx->d_counts, ctx->d_next, ctx->d_aerr);
  if (int rc = check_launch(ctx, "ldg_k_audio_ds")) return rc;
  return audio_out(ctx, s, n, pcm, pcm_stride, counts, next_offsets);
}

// ---- RF dropouts (dropout.hip; build-defined, DESIGN.md section 7) ----------------
int ldg_dropout_defaults(int system, ldg_dropout_opts* out) {
  if (!out || (system != LDG_SYSTEM_NTSC && system != LDG_SYSTEM_PAL)) return LDG_EINVAL;
  const double vsync_ire = system == LDG_SYSTEM_PAL ? -.3 * (100 / .7) : -40.0;
  out->lo_ire = vsync_ire - 50;
  out->hi_ire = 150;
  out->merge_gap = 80;
  out->min_flagged = 3;
  out->pad = 24;
  out->conceal = 0;
  return LDG_OK;
}

static int drop_alloc(ldg_ctx* ctx) {
  if (ctx->d_drop_runs) return LDG_OK;
  const size_t R = (size_t)ctx->max_reads, F = 2 * (size_t)ctx->max_frames;
  int rc = 0;
  rc |= dmalloc(ctx, &ctx->d_drop_cnt, R * MAX_LINES);
  rc |= dmalloc(ctx, &ctx->d_drop_rows, R);
  rc |= dmalloc(ctx, &ctx->d_drop_map, R);
  rc |= dmalloc(ctx, &ctx->d_fdrop_runs, F * DROP_RUNS_STRIDE);
  rc |= dmalloc(ctx, &ctx->d_fdrop_cnt, F * MAX_LINES);
  rc |= dmalloc(ctx, &ctx->d_fdrop_rows, F);
  rc |= dmalloc(ctx, &ctx->d_fdrop_map, F);
  if (!rc && hipHostMalloc((void**)&ctx->h_drop, R * (DROP_RUNS_STRIDE * sizeof(int16_t) + (MAX_LINES + 1) * sizeof(int32_t)),
                           hipHostMallocDefault) != hipSuccess)
    rc |= LDG_ENOMEM;
  rc |= dmalloc(ctx, &ctx->d_drop_runs, R * DROP_RUNS_STRIDE);     // last: marks the set complete
  if (rc) {
    for (void** p : {(void**)&ctx->d_drop_runs, (void**)&ctx->d_fdrop_runs, (void**)&ctx->d_drop_cnt, (void**)&ctx->d_drop_rows,
                     (void**)&ctx->d_fdrop_cnt, (void**)&ctx->d_fdrop_rows, (void**)&ctx->d_drop_map, (void**)&ctx->d_fdrop_map}) {
      dfree(*p);
      *p = nullptr;
    }
    if (ctx->h_drop) (void)hipHostFree(ctx->h_drop);
    ctx->h_drop = nullptr;
    ctx->err = "dropout buffers: out of memory";
    return LDG_ENOMEM;
  }
  // a slot never detected reads as "not valid", its rows as empty
  LDG_TRY(hipMemset(ctx->d_drop_rows, 0xff, R * sizeof(int32_t)));
  LDG_TRY(hipMemset(ctx->d_drop_cnt, 0, R * MAX_LINES * sizeof(int32_t)));
  LDG_TRY(hipMemset(ctx->d_drop_runs, 0, R * DROP_RUNS_STRIDE * sizeof(int16_t)));
  return LDG_OK;
}

int ldg_set_dropout_opts(ldg_ctx* ctx, const ldg_dropout_opts* o) {
  if (!ctx) return LDG_EINVAL;
  if (!o) {
    ctx->drop_on = false;
    return LDG_OK;
  }
  if (!(o->lo_ire <= o->hi_ire) || o->merge_gap < 1 || o->merge_gap > (1 << 20) || o->min_flagged < 1 || o->pad < 0 ||
      o->pad > (1 << 20)) {
    ctx->err = "ldg_set_dropout_opts: lo_ire <= hi_ire, merge_gap >= 1, min_flagged >= 1, pad >= 0";
    return LDG_EINVAL;
  }
  LDG_TRY(hipSetDevice(ctx->device));
  if (int rc = drop_alloc(ctx)) return rc;
  ctx->drop_opts = *o;
  ctx->drop_on = true;
  return LDG_OK;
}

// ldg_k_dropout_lines over n slots (device map) on stream s
static int drop_detect(ldg_ctx* ctx, hipStream_t s, int n, const int32_t* d_map, int by_slot, int16_t* runs,
                       int32_t* counts, int32_t* nrows) {
  const SysConst& C = ctx->C;
  DropParams P;
  P.lo_hz = C.ire0 + C.hz_ire * ctx->drop_opts.lo_ire;
  P.hi_hz = C.ire0 + C.hz_ire * ctx->drop_opts.hi_ire;
  P.merge_gap = ctx->drop_opts.merge_gap;
  P.min_flagged = ctx->drop_opts.min_flagged;
  P.pad = ctx->drop_opts.pad;
  P.pad_ = 0;
  const dim3 g_rows((unsigned)(C.frame_lines / 2 + 1), (unsigned)n);     // as ldg_k_final_lines
  LDG_LAUNCH_ON(s, "dropout_lines", ldg_k_dropout_lines, g_rows, 64, d_map, by_slot, ctx->video, ctx->vread, ctx->vchan,
                C, ctx->d_recs, ctx->d_lines, P, runs, counts, nrows);
  return check_launch(ctx, "ldg_k_dropout_lines");
}

int ldg_field_dropouts(ldg_ctx* ctx, int n, const int32_t* slots, ldg_dropout* out, int64_t out_stride,
                       int32_t* counts) {
  if (!ctx || n < 0 || n > ctx->max_reads || (n && (!slots || !out || !counts)) || out_stride < 0) return LDG_EINVAL;
  if (!ctx->drop_on) {
    ctx->err = "ldg_field_dropouts: the dropout options are off (ldg_set_dropout_opts)";
    return LDG_ESTATE;
  }
  if (n == 0) return LDG_OK;
  int lo = ctx->max_reads, hi = -1;
  for (int i = 0; i < n; i++) {
    if (slots[i] < 0 || slots[i] >= ctx->max_reads || !ctx->live[slots[i]]) return LDG_EINVAL;
    lo = std::min(lo, (int)slots[i]);
    hi = std::max(hi, (int)slots[i]);
  }
  LDG_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->sout;     // output work: overlaps the outstanding decodes
  if (int rc = stage_h2d(ctx, ctx->d_drop_map, slots, n * sizeof(int32_t), s)) return rc;
  if (int rc = drop_detect(ctx, s, n, ctx->d_drop_map, 1, ctx->d_drop_runs, ctx->d_drop_cnt, ctx->d_drop_rows)) return rc;
  // the slots' span of the three arrays in one copy each
  const size_t m = (size_t)(hi - lo + 1);
  int16_t* h_runs = (int16_t*)ctx->h_drop;
  int32_t* h_cnt = (int32_t*)(h_runs + (size_t)ctx->max_reads * DROP_RUNS_STRIDE);
  int32_t* h_rows = h_cnt + (size_t)ctx->max_reads * MAX_LINES;
  LDG_TRY(hipMemcpyAsync(h_runs, ctx->d_drop_runs + (size_t)lo * DROP_RUNS_STRIDE, m * DROP_RUNS_STRIDE * sizeof(int16_t),
                         hipMemcpyDeviceToHost, s));
  LDG_TRY(hipMemcpyAsync(h_cnt, ctx->d_drop_cnt + (size_t)lo * MAX_LINES, m * MAX_LINES * sizeof(int32_t),
                         hipMemcpyDeviceToHost, s));
  LDG_TRY(hipMemcpyAsync(h_rows, ctx->d_drop_rows + lo, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LDG_TRY(hipStreamSynchronize(s));
  prof_collect(ctx);
  for (int i = 0; i < n; i++) {
    const size_t e = (size_t)(slots[i] - lo);
    const int rows = h_rows[e];
    if (rows < 0) {
      counts[i] = -1;
      continue;
    }
    ldg_dropout* o = out + (size_t)i * out_stride;
    int64_t k = 0;
    for (int r = 0; r < rows && r < MAX_LINES; r++) {
      const int c = std::min<int>(std::max<int>(h_cnt[e * MAX_LINES + r], 0), MAX_DROPOUTS);
      for (int q = 0; q < c; q++) {
        if (k >= out_stride) {
          ctx->err = "ldg_field_dropouts: out_stride is too small for a field's runs";
          return LDG_EINVAL;
        }
        const int16_t* p = h_runs + e * DROP_RUNS_STRIDE + ((size_t)r * MAX_DROPOUTS + q) * 2;
        o[k++] = ldg_dropout{(int16_t)r, p[0], p[1], 0};
      }
    }
    counts[i] = (int32_t)k;
  }
  return LDG_OK;
}

// ---- disc stacking (stack.hip; build-defined, DESIGN.md section 7b) ----------------
static void stack_free(ldg_ctx* ctx) {
  if (ctx->sstack) {
    (void)hipStreamSynchronize(ctx->sstack);
    (void)hipStreamDestroy(ctx->sstack);
    ctx->sstack = nullptr;
  }
  for (void** p : {(void**)&ctx->d_stack_src, (void**)&ctx->d_stack_out, (void**)&ctx->d_stack_runs,
                   (void**)&ctx->d_stack_cnt, (void**)&ctx->d_stack_rows, (void**)&ctx->d_stack_rowinfo}) {
    dfree(*p);
    *p = nullptr;
  }
  ctx->stack_cap = 0;
}

static size_t stack_frame_px(const ldg_ctx* ctx) { return ctx->system == 1 ? (size_t)1135 * 625 : (size_t)910 * 525; }

// staging for n_src sources of max_frames frames, their runs, and the output frames
static int stack_alloc(ldg_ctx* ctx, int n_src) {
  if (ctx->stack_cap >= n_src) return LDG_OK;
  stack_free(ctx);
  if (hipStreamCreateWithFlags(&ctx->sstack, hipStreamNonBlocking) != hipSuccess) {
    ctx->sstack = nullptr;
    ctx->err = "stacking: hipStreamCreate failed";
    return LDG_EDEVICE;
  }
  const size_t F = (size_t)ctx->max_frames, S = (size_t)n_src;
  ctx->stack_src_stride = (int64_t)((F * stack_frame_px(ctx) + 7) & ~(size_t)7);
  int rc = 0;
  rc |= dmalloc(ctx, &ctx->d_stack_src, S * (size_t)ctx->stack_src_stride);
  rc |= dmalloc(ctx, &ctx->d_stack_out, F * stack_frame_px(ctx));
  rc |= dmalloc(ctx, &ctx->d_stack_runs, F * S * 2 * STACK_RUNS_STRIDE);
  rc |= dmalloc(ctx, &ctx->d_stack_cnt, F * S * 2 * MAX_LINES);
  rc |= dmalloc(ctx, &ctx->d_stack_rows, F * 2);
  rc |= dmalloc(ctx, &ctx->d_stack_rowinfo, F * 625);
  if (rc) {
    stack_free(ctx);
    ctx->err = "stacking buffers: out of memory";
    return LDG_ENOMEM;
  }
  ctx->stack_cap = n_src;
  return LDG_OK;
}

int ldg_stack_frames(ldg_ctx* ctx, int n_frames, int n_src, const uint16_t* const* src, const uint8_t* present,
                     const int16_t* runs, const int32_t* counts, int mode, int threshold, uint16_t* out) {
  if (!ctx) return LDG_EINVAL;
  auto bad = [&](const char* what) {
    ctx->err = std::string("ldg_stack_frames: ") + what;
    return LDG_EINVAL;
  };
  if (n_src < 1 || n_src > LDG_STACK_MAX_SOURCES) return bad("n_src must be 1..16");
  if (n_frames < 0 || n_frames > ctx->max_frames) return bad("n_frames must be 0..max_frames");
  if (mode != LDG_STACK_MEDIAN && mode != LDG_STACK_MEAN && mode != LDG_STACK_SMART_MEAN)
    return bad("mode must be LDG_STACK_MEDIAN, LDG_STACK_MEAN or LDG_STACK_SMART_MEAN");
  if (threshold < 0 || threshold > 65535) return bad("threshold must be 0..65535");
  if (n_frames == 0) return LDG_OK;
  if (!src || !present || !out) return bad("src, present and out must not be NULL");
  if ((runs == nullptr) != (counts == nullptr)) return bad("runs and counts must both be given or both be NULL");
  for (int f = 0; f < n_frames; f++) {
    bool any = false;
    for (int s = 0; s < n_src; s++) {
      if (!present[(size_t)f * n_src + s]) continue;
      any = true;
      if (!src[s]) return bad("src[s] is NULL for a source that present marks");
    }
    if (!any) return bad("present: a frame has no present source");
  }
  LDG_TRY(hipSetDevice(ctx->device));
  if (int rc = stack_alloc(ctx, n_src)) return rc;
  hipStream_t st = ctx->sstack;
  const size_t fpx = stack_frame_px(ctx);
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = now();
  // each source's runs of consecutive present frames, packed as in the file
  for (int s = 0; s < n_src; s++) {
    for (int f = 0; f < n_frames;) {
      if (!present[(size_t)f * n_src + s]) {
        f++;
        continue;
      }
      int e = f + 1;
      while (e < n_frames && present[(size_t)e * n_src + s]) e++;
      LDG_TRY(hipMemcpyAsync(ctx->d_stack_src + (size_t)s * ctx->stack_src_stride + (size_t)f * fpx, src[s] + (size_t)f * fpx,
                             (size_t)(e - f) * fpx * sizeof(uint16_t), hipMemcpyHostToDevice, st));
      f = e;
    }
  }
  // per frame row: the sources present (bits 0..15) and whether one of them has a run there (bit 31)
  const int H = ctx->system == 1 ? 625 : 525;
  std::vector<uint32_t> rowinfo((size_t)n_frames * H);
  for (int f = 0; f < n_frames; f++) {
    uint32_t pm = 0;
    for (int s = 0; s < n_src; s++)
      if (present[(size_t)f * n_src + s]) pm |= 1u << s;
    uint32_t* ri = rowinfo.data() + (size_t)f * H;
    for (int y = 0; y < H; y++) ri[y] = pm;
    if (!counts) continue;
    for (int s = 0; s < n_src; s++) {
      if (!((pm >> s) & 1u)) continue;
      const int32_t* c = counts + ((size_t)f * n_src + s) * 2 * MAX_LINES;
      for (int p = 0; p < 2; p++)
        for (int r = 0; 2 * r + p < H; r++)
          if (c[p * MAX_LINES + r] > 0) ri[2 * r + p] |= 1u << 31;
    }
  }
  LDG_TRY(hipMemcpyAsync(ctx->d_stack_rowinfo, rowinfo.data(), rowinfo.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (runs) {
    const size_t E = (size_t)n_frames * n_src * 2;
    LDG_TRY(hipMemcpyAsync(ctx->d_stack_runs, runs, E * STACK_RUNS_STRIDE * sizeof(int16_t), hipMemcpyHostToDevice, st));
    LDG_TRY(hipMemcpyAsync(ctx->d_stack_cnt, counts, E * MAX_LINES * sizeof(int32_t), hipMemcpyHostToDevice, st));
  }
  LDG_TRY(hipStreamSynchronize(st));
  const double t1 = now();
  StackArgs A;
  A.src = ctx->d_stack_src;
  A.src_stride = ctx->stack_src_stride;
  A.rowinfo = ctx->d_stack_rowinfo;
  A.runs = runs ? ctx->d_stack_runs : nullptr;
  A.counts = runs ? ctx->d_stack_cnt : nullptr;
  A.out = ctx->d_stack_out;
  A.n_src = n_src;
  A.W = ctx->system == 1 ? 1135 : 910;
  A.H = H;
  A.ntsc = ctx->system == 0;
  A.mode = mode;
  A.threshold = threshold;
  const dim3 grid((unsigned)A.H, (unsigned)n_frames);
  // the kernel unrolled for the next size that holds n_src (the slots past n_src are absent)
  if (n_src <= 1) stack_launch<1>(ctx, st, grid, A);
  else if (n_src <= 2) stack_launch<2>(ctx, st, grid, A);
  else if (n_src <= 3) stack_launch<3>(ctx, st, grid, A);
  else if (n_src <= 4) stack_launch<4>(ctx, st, grid, A);
  else if (n_src <= 6) stack_launch<6>(ctx, st, grid, A);
  else if (n_src <= 8) stack_launch<8>(ctx, st, grid, A);
  else if (n_src <= 12) stack_launch<12>(ctx, st, grid, A);
  else stack_launch<16>(ctx, st, grid, A);
  if (int rc = check_launch(ctx, "ldg_k_stack")) return rc;
  LDG_TRY(hipStreamSynchronize(st));
  const double t2 = now();
  LDG_TRY(hipMemcpyAsync(out, ctx->d_stack_out, (size_t)n_frames * fpx * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
  LDG_TRY(hipStreamSynchronize(st));
  const double t3 = now();
  ctx->stack_t[0] += t1 - t0;
  ctx->stack_t[1] += t2 - t1;
  ctx->stack_t[2] += t3 - t2;
  ctx->stack_t[3] += 1;
  prof_collect(ctx);
  return LDG_OK;
}

int ldg_stack_stats(ldg_ctx* ctx, double* out, int n) {
  if (!ctx || !out || n < 0) return LDG_EINVAL;
  const int m = n < 4 ? n : 4;
  for (int i = 0; i < m; i++) out[i] = ctx->stack_t[i];
  return m;
}

int ldg_conceal_frames(ldg_ctx* ctx, int n, uint16_t* frames, const int16_t* runs, const int32_t* counts,
                       const int32_t* nrows) {
  if (!ctx) return LDG_EINVAL;
  if (n < 0 || (n && (!frames || !runs || !counts || !nrows))) {
    ctx->err = "ldg_conceal_frames: n >= 0; frames, runs, counts and nrows must not be NULL";
    return LDG_EINVAL;
  }
  for (int i = 0; i < 2 * n; i++)
    if (nrows[i] < -1 || nrows[i] > MAX_LINES) {
      ctx->err = "ldg_conceal_frames: nrows must be -1..320";
      return LDG_EINVAL;
    }
  if (n == 0) return LDG_OK;
  LDG_TRY(hipSetDevice(ctx->device));
  if (int rc = stack_alloc(ctx, 1)) return rc;
  hipStream_t st = ctx->sstack;
  const size_t fpx = stack_frame_px(ctx);
  SysConst C{};                    // what ldg_k_conceal reads of it
  C.system = ctx->system;
  C.outlinelen = ctx->system == 1 ? 1135 : 910;
  C.frame_lines = ctx->system == 1 ? 625 : 525;
  for (int done = 0; done < n;) {
    const int m = (n - done) < ctx->max_frames ? (n - done) : ctx->max_frames;
    uint16_t* h = frames + (size_t)done * fpx;
    LDG_TRY(hipMemcpyAsync(ctx->d_stack_out, h, m * fpx * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    LDG_TRY(hipMemcpyAsync(ctx->d_stack_runs, runs + (size_t)done * 2 * STACK_RUNS_STRIDE,
                           (size_t)m * 2 * STACK_RUNS_STRIDE * sizeof(int16_t), hipMemcpyHostToDevice, st));
    LDG_TRY(hipMemcpyAsync(ctx->d_stack_cnt, counts + (size_t)done * 2 * MAX_LINES, (size_t)m * 2 * MAX_LINES * sizeof(int32_t),
                           hipMemcpyHostToDevice, st));
    LDG_TRY(hipMemcpyAsync(ctx->d_stack_rows, nrows + (size_t)done * 2, (size_t)m * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    LDG_LAUNCH_ON(st, "conceal", ldg_k_conceal, dim3((unsigned)C.frame_lines, (unsigned)m), 64, ctx->d_stack_runs,
                  ctx->d_stack_cnt, ctx->d_stack_rows, C, ctx->d_stack_out);
    if (int rc = check_launch(ctx, "ldg_k_conceal")) return rc;
    LDG_TRY(hipMemcpyAsync(h, ctx->d_stack_out, m * fpx * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    LDG_TRY(hipStreamSynchronize(st));
    done += m;
  }
  prof_collect(ctx);
  return LDG_OK;
}

int ldg_assemble_frames(ldg_ctx* ctx, int n, const int32_t* top_slots, const int32_t* bottom_slots, uint16_t* out,
                        int out_is_device) {
  // out == NULL with out_is_device: frames stay in the context's internal device frame buffer
  if (!ctx || n < 0 || n > ctx->max_frames || (n && (!top_slots || !bottom_slots || (!out && !out_is_device))))
    return LDG_EINVAL;
  if (n == 0) return LDG_OK;
  for (int i = 0; i < n; i++)
    if (top_slots[i] < 0 || top_slots[i] >= ctx->max_reads || bottom_slots[i] < 0 ||
        bottom_slots[i] >= ctx->max_reads || !ctx->live[top_slots[i]] || !ctx->live[bottom_slots[i]])
      return LDG_EINVAL;
  LDG_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream2;   // output work: overlaps the outstanding decodes
  if (int rc = stage_h2d(ctx, ctx->d_slots, top_slots, n * sizeof(int32_t), s)) return rc;
  if (int rc = stage_h2d(ctx, ctx->d_slots2, bottom_slots, n * sizeof(int32_t), s)) return rc;
  const size_t fsz = (size_t)ctx->C.frame_lines * ctx->C.outlinelen;
  uint16_t* dst = out;
  if (!(out_is_device && out)) {
    // the context's frame buffers alternate; wait for the last reader of the one written now
    ctx->fb ^= 1;
    if (ctx->fbuf_recorded[ctx->fb]) LDG_TRY(hipStreamWaitEvent(s, ctx->ev_fbuf[ctx->fb], 0));
    dst = ctx->frame_buf(ctx->fb);
  }
  const bool conceal = ctx->drop_on && ctx->drop_opts.conceal;
  if (conceal) {
    // the fields' runs (entry 2 f + parity), while their slots are still protected
    std::vector<int32_t> map(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
      map[2 * i] = top_slots[i];
      map[2 * i + 1] = bottom_slots[i];
    }
    if (int rc = stage_h2d(ctx, ctx->d_fdrop_map, map.data(), map.size() * sizeof(int32_t), s)) return rc;
    if (int rc = drop_detect(ctx, s, 2 * n, ctx->d_fdrop_map, 0, ctx->d_fdrop_runs, ctx->d_fdrop_cnt, ctx->d_fdrop_rows))
      return rc;
  }
  dim3 grid(n, (ctx->C.frame_lines + FRAME_ROWS - 1) / FRAME_ROWS);
  LDG_LAUNCH_ON(s, "frames", ldg_k_frames, grid, 256, ctx->d_slots, ctx->d_slots2, ctx->d_recs, ctx->d_pic,
             ctx->pic_stride, ctx->C, dst);
  if (int rc = check_launch(ctx, "ldg_k_frames")) return rc;
  if (conceal) {
    // in place, before the comb or any copy sees the frames (both wait for ev_frames / this stream)
    LDG_LAUNCH_ON(s, "conceal", ldg_k_conceal, dim3((unsigned)ctx->C.frame_lines, (unsigned)n), 64, ctx->d_fdrop_runs,
                  ctx->d_fdrop_cnt, ctx->d_fdrop_rows, ctx->C, dst);
    if (int rc = check_launch(ctx, "ldg_k_conceal")) return rc;
  }
  // the next decode's field chains (which rewrite slots) wait for this
  LDG_TRY(hipEventRecord(ctx->ev_frames, s));
  ctx->frames_recorded = true;
  if (conceal) ctx->frames_demod = true;
  if (out_is_device) return LDG_OK;      // stays queued on the output stream
  LDG_TRY(hipMemcpyAsync(out, dst, n * fsz * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
  LDG_TRY(hipStreamSynchronize(s));
  prof_collect(ctx);
  return LDG_OK;
}

// the asynchronous comb's work done (its stream and the output stream drained)
static int comb_quiesce(ldg_ctx* ctx) {
  LDG_TRY(hipSetDevice(ctx->device));
  LDG_TRY(hipStreamSynchronize(ctx->scomb));
  LDG_TRY(hipStreamSynchronize(ctx->stream2));
  ctx->comb_pending = false;
  return LDG_OK;
}

// ---- asynchronous host output (the CLI's .tbc / .rgb path) -----------------------
static int comb_alloc(ldg_ctx* ctx);
static int pal_alloc(ldg_ctx* ctx);
static int pal_launch(ldg_ctx* ctx, hipStream_t s, const uint16_t* src, int m);
static int comb_launch(ldg_ctx* ctx, hipStream_t st, const uint16_t* src, int n, uint16_t* dst, bool d3 = false,
                       double core = 0, double range = 1, const double* kmap = nullptr);

int ldg_output_async(ldg_ctx* ctx, int n, const int32_t* top_slots, const int32_t* bottom_slots, uint16_t* tbc_host,
                     uint16_t* rgb_host) {
  if (!ctx || n < 0 || n > ctx->max_frames || !tbc_host) return LDG_EINVAL;
  if (n == 0) return LDG_OK;
  if (ctx->out_n == ldg_ctx::OUT_Q) { ctx->err = "output_async: 4 calls outstanding (ldg_output_wait first)"; return LDG_ESTATE; }
  const bool pal_rgb = ctx->have_filters && ctx->C.system == 1;
  // frames into the device frame buffer on the output stream (ev_frames for the slot readers)
  if (int rc = ldg_assemble_frames(ctx, n, top_slots, bottom_slots, nullptr, 1)) return rc;
  hipStream_t s = ctx->stream2;
  const size_t fsz = (size_t)ctx->C.frame_lines * ctx->C.outlinelen;
  const int b = ctx->fb;
  LDG_TRY(hipMemcpyAsync(tbc_host, ctx->frame_buf(b), n * fsz * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
  if (rgb_host) {
    // the comb on its own stream after this assembly; the output event and the
    // buffer's reader event go behind both the comb's and the .tbc copy
    if (int rc = pal_rgb ? pal_alloc(ctx) : comb_alloc(ctx)) return rc;
    hipStream_t c = ctx->scomb;
    LDG_TRY(hipEventRecord(ctx->ev_tbc, s));
    LDG_TRY(hipStreamWaitEvent(c, ctx->ev_frames, 0));
    if (pal_rgb) {
      // the PAL Y/C decoder (build-defined, row F2): 576 x 1057 rgb48 per frame
      if (int rc = pal_launch(ctx, c, ctx->frame_buf(b), n)) return rc;
      const size_t fout = (size_t)pal::OUT_W * pal::OUT_H * 3;
      LDG_TRY(hipMemcpyAsync(rgb_host, ctx->pal_rgb, n * fout * sizeof(uint16_t), hipMemcpyDeviceToHost, c));
    } else {
      if (int rc = comb_launch(ctx, c, ctx->frame_buf(b), n, ctx->comb_rgb)) return rc;
      const size_t fout = (size_t)ctx->comb_opt.out_w() * ctx->comb_opt.out_rows * 3;
      LDG_TRY(hipMemcpyAsync(rgb_host, ctx->comb_rgb, n * fout * sizeof(uint16_t), hipMemcpyDeviceToHost, c));
    }
    LDG_TRY(hipStreamWaitEvent(c, ctx->ev_tbc, 0));
    ctx->comb_pending = true;
    s = c;
  }
  LDG_TRY(hipEventRecord(ctx->ev_fbuf[b], s));
  ctx->fbuf_recorded[b] = true;
  LDG_TRY(hipEventRecord(ctx->ev_outq[(ctx->out_head + ctx->out_n) % ldg_ctx::OUT_Q], s));
  ctx->out_n++;
  return LDG_OK;
}

int ldg_output_wait(ldg_ctx* ctx) {
  if (!ctx) return LDG_EINVAL;
  if (!ctx->out_n) return LDG_OK;
  LDG_TRY(hipSetDevice(ctx->device));
  LDG_TRY(hipEventSynchronize(ctx->ev_outq[ctx->out_head]));
  ctx->out_head = (ctx->out_head + 1) % ldg_ctx::OUT_Q;
  ctx->out_n--;
  return LDG_OK;
}

int ldg_host_alloc(int64_t nbytes, void** out) {
  if (!out || nbytes <= 0) return LDG_EINVAL;
  *out = nullptr;
  if (hipHostMalloc(out, (size_t)nbytes, hipHostMallocDefault) != hipSuccess) return LDG_ENOMEM;
  return LDG_OK;
}

int ldg_host_free(void* p) {
  if (p && hipHostFree(p) != hipSuccess) return LDG_EDEVICE;
  return LDG_OK;
}

// ---- 2D NTSC comb (comb-ntsc.cxx dim=2; options: ldg_comb_set_opts) ------------
static int comb_alloc(ldg_ctx* ctx) {
  if (ctx->comb_state) return LDG_OK;
  const size_t F = (size_t)ctx->max_frames;
  int rc = 0;
  rc |= dmalloc(ctx, &ctx->comb_state, 1);
  rc |= dmalloc(ctx, &ctx->comb_abl, F * comb::CHAIN_MAX);
  rc |= dmalloc(ctx, &ctx->comb_in, F * comb::IN_X * comb::IN_Y);
  rc |= dmalloc(ctx, &ctx->comb_rgb, F * comb::IN_X * comb::OUT_HMAX * 3);    // -W: 910 wide
  rc |= dmalloc(ctx, &ctx->comb_hist, 24);
  rc |= dmalloc(ctx, &ctx->comb_cv, F * comb::ROWS_MAX * comb::CV_STRIDE);
  rc |= dmalloc(ctx, &ctx->comb_iqo, F * comb::IQ_ROWS_MAX * 2 * comb::IQ_NS);
  if (rc) return LDG_ENOMEM;
  const double init = -1.0;
  LDG_TRY(hipMemcpy(ctx->comb_state, &init, sizeof(double), hipMemcpyHostToDevice));
  LDG_TRY(hipMemset(ctx->comb_hist, 0, 24 * sizeof(double)));
  ctx->comb_hist_cur = 0;
  return LDG_OK;
}

// the comb's kernel sequence over n frames at `src` (device) into rgb48 `dst`;
// d3: the 3D split (src[-1] and src[n] are the outer frames' neighbours)
static int comb_launch(ldg_ctx* ctx, hipStream_t st, const uint16_t* src, int n, uint16_t* dst, bool d3,
                       double core, double range, const double* kmap) {
  comb::CombOpt O = ctx->comb_opt;
  if (kmap) {
    // the flow path's DoYNR(0, tbuf, 4) / DoCNR(0, tbuf, 4) raise the global clips to at
    // least 4 (raw units) from the second frame on, so every output sees them (comb-ntsc.cxx:
    // 487-488, 527-529, 853-855)
    if (O.nr_y < 4) O.nr_y = 4;
    if (O.nr_c < 4) O.nr_c = 4;
  }
  LDG_LAUNCH_ON(st, "comb_burst", ldg_k_comb_burst, 1, 256, src, n, ctx->comb_state, ctx->comb_abl, ctx->comb_warm,
                O.firstline);
  ctx->comb_last_lines = n * O.chain_lines();
  if (d3 && kmap)
    LDG_LAUNCH_ON(st, "comb_split3", ldg_k_comb_split3_of, n * O.nrows, 256, src, ctx->comb_cv, O, kmap);
  else if (d3)
    LDG_LAUNCH_ON(st, "comb_split3", ldg_k_comb_split3, n * O.nrows, 256, src, ctx->comb_cv, core, range, O);
  const bool def = !ctx->comb_generic && comb_is_default(O);
  if (!d3 && def && !ctx->comb_unfused) {
    // the default 2D comb: split, FilterIQ and output in one row kernel (cv in LDS)
    const int total = n * O.nrows;
    LDG_LAUNCH_ON(st, "comb_fused", ldg_k_comb_fused, total, 256, src, ctx->comb_abl, dst, ctx->comb_iqw);
    return check_launch(ctx, "comb kernels");
  }
  if (!d3 && def)
    LDG_LAUNCH_ON(st, "comb_split", ldg_k_comb_split, n * O.nrows, 256, src, ctx->comb_cv);
  else if (!d3)
    LDG_LAUNCH_ON(st, "comb_split", ldg_k_comb_split_opt, n * O.nrows, 256, src, ctx->comb_cv, O);
  if (O.colorlpf && def)
    LDG_LAUNCH_ON(st, "comb_iq", ldg_k_comb_iq, (n * O.iq_rows() * 2 + 255) / 256, 256, ctx->comb_cv, n,
                  ctx->comb_iqo);
  else if (O.colorlpf)
    LDG_LAUNCH_ON(st, "comb_iq", ldg_k_comb_iq_opt, (n * O.iq_rows() * 2 + 255) / 256, 256, ctx->comb_cv, n,
                  ctx->comb_iqo, O);
  if (def)
    LDG_LAUNCH_ON(st, "comb_out", ldg_k_comb_out, n * O.out_rows, 256, src, ctx->comb_cv, ctx->comb_iqo,
                  ctx->comb_abl, dst);
  else {
    // -W: DoYNR's history enters from the previous call and leaves for the next
    const double* hin = ctx->comb_hist + 12 * ctx->comb_hist_cur;
    double* hout = ctx->comb_hist + 12 * (ctx->comb_hist_cur ^ 1);
    LDG_LAUNCH_ON(st, "comb_out", ldg_k_comb_out_opt, n * O.out_rows, 256, src, ctx->comb_cv, ctx->comb_iqo,
                  ctx->comb_abl, dst, O, hin, hout, n);
    ctx->comb_hist_cur ^= 1;
  }
  return check_launch(ctx, "comb kernels");
}

int ldg_comb_set_opts(ldg_ctx* ctx, const ldg_comb_opts* o) {
  if (!ctx) return LDG_EINVAL;
  comb::CombOpt c = comb_defaults();
  if (o) {
    if (o->linesout != 480 && o->linesout != 525) { ctx->err = "comb: linesout must be 480 or 525"; return LDG_EINVAL; }
    if (o->black_ire == 100.0) { ctx->err = "comb: black_ire 100 divides by zero"; return LDG_EINVAL; }
    c.firstline = (o->linesout == comb::IN_Y) ? 20 : 38;              // comb-ntsc.cxx:486,524,736,836
    c.nrows = comb::IN_Y - c.firstline < o->linesout ? comb::IN_Y - c.firstline : o->linesout;
    c.out_rows = o->linesout;
    c.adaptive2d = o->adaptive2d ? 1 : 0;
    c.bw = o->bw ? 1 : 0;
    c.colorlpf = o->colorlpf ? 1 : 0;
    c.lpq = o->colorlpf_hq ? 0 : 1;
    const int dr = o->debug_line + 25 - c.firstline;                  // ToRGB: l == f_debugline + 25
    c.debug_row = (dr >= 0 && dr < c.nrows) ? dr : -1;
    c.black_ire = o->black_ire;
    c.bright_m = o->brightness * 256 / 100;
    c.nr_y = o->nr_y * comb::IRESCALE;                                // main(): nr_y *= irescale
    c.nr_c = o->nr_c * comb::IRESCALE;
    c.wide = o->wide ? 1 : 0;
    c.of = o->opticalflow ? 1 : 0;
    // -W: combed rows run to line 524 (DoYNR feeds every line; its history reaches x 40..51)
    if (c.wide) c.nrows = comb::IN_Y - c.firstline;
  }
  LDG_TRY(hipSetDevice(ctx->device));
  if (int rc = comb_quiesce(ctx)) return rc;
  ctx->comb_opt = c;
  return LDG_OK;
}

int ldg_comb_reset(ldg_ctx* ctx) {
  if (!ctx) return LDG_EINVAL;
  LDG_TRY(hipSetDevice(ctx->device));
  if (int rc = comb_quiesce(ctx)) return rc;
  ctx->comb3_hist = 0;
  ctx->of.frames = 0;
  ctx->of.rcur = 0;
  if (int rc = comb_alloc(ctx)) return rc;
  const double init = -1.0;
  LDG_TRY(hipMemcpy(ctx->comb_state, &init, sizeof(double), hipMemcpyHostToDevice));
  LDG_TRY(hipMemset(ctx->comb_hist, 0, 24 * sizeof(double)));
  ctx->comb_hist_cur = 0;
  if (ctx->pal_state) {
    const double init2[2] = {-1.0, -1.0};
    LDG_TRY(hipMemcpy(ctx->pal_state, init2, sizeof(init2), hipMemcpyHostToDevice));
    ctx->pal_scur = 0;
  }
  return LDG_OK;
}

int ldg_comb_set_state(ldg_ctx* ctx, double aburstlev) {
  if (!ctx) return LDG_EINVAL;
  LDG_TRY(hipSetDevice(ctx->device));
  if (int rc = comb_quiesce(ctx)) return rc;
  if (int rc = comb_alloc(ctx)) return rc;
  LDG_TRY(hipMemcpy(ctx->comb_state, &aburstlev, sizeof(double), hipMemcpyHostToDevice));
  return LDG_OK;
}

// Benchmark roofline leg: the demod alone over n live slots, `iters` launches back
// to back on the context's stream, HIP events around each.  variant 0:
// ldg_k_demod_iso (every block in full); 1: ldg_k_demod_iso_cut, the production
// body (demod_body<true>: blocks past a read's video cut stop after the sync
// channel) under its own symbol.
int ldg_demod_isolated_ex(ldg_ctx* ctx, int n, const int32_t* slots, int iters, int variant, double* ms_per_launch) {
  if (!ctx || !slots || n <= 0 || n > ctx->max_reads || iters <= 0 || !ms_per_launch) return LDG_EINVAL;
  if (variant != 0 && variant != 1) return LDG_EINVAL;
  for (int i = 0; i < n; i++)
    if (slots[i] < 0 || slots[i] >= ctx->max_reads || !ctx->live[slots[i]]) return LDG_EINVAL;
  LDG_TRY(hipSetDevice(ctx->device));
  LDG_TRY(hipDeviceSynchronize());
  if (!ctx->d_isomap) {
    if (int rc = dmalloc(ctx, &ctx->d_isomap, (size_t)ctx->max_reads)) return rc;
  }
  LDG_TRY(hipMemcpy(ctx->d_isomap, slots, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
  // the leg times whole reads: a read with a block outside the resident capture (a
  // speculative read past a sharded rank's window: FS_EOF, its workgroups return at
  // once) would be counted as a full read's samples, so such reads are refused
  std::vector<int32_t> st_h((size_t)ctx->max_reads);
  LDG_TRY(hipMemcpy(st_h.data(), ctx->d_status, st_h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++)
    if (st_h[slots[i]] == FS_EOF) { ctx->err = "demod_isolated: a read lies outside the resident capture"; return LDG_ESTATE; }
  // the reads' filter tables came from several calls: the leg gives every table index a
  // read uses a copy of one valid table (the last call's first), so its timing runs on
  // real filter values
  if (!ctx->rf_cur) { ctx->err = "demod_isolated: no decode yet"; return LDG_ESTATE; }
  int nt = 1;
  for (int i = 0; i < n; i++) nt = std::max(nt, ctx->h_reads[slots[i]].filt_slot + 1);
  if (ctx->rf_iso_cap < nt) {
    dfree(ctx->rf_iso);
    ctx->rf_iso = nullptr;
    ctx->rf_iso_cap = 0;
    if (int rc = dmalloc(ctx, &ctx->rf_iso, (size_t)nt * BLOCKLEN)) return rc;
    ctx->rf_iso_cap = nt;
  }
  for (int t = 0; t < nt; t++)
    LDG_TRY(hipMemcpy(ctx->rf_iso + (size_t)t * BLOCKLEN, ctx->rf_cur, BLOCKLEN * sizeof(double2),
                      hipMemcpyDeviceToDevice));
  const SysConst C = ctx->C;
  hipStream_t st = ctx->stream;
  std::vector<hipEvent_t> ev(2 * (size_t)iters, nullptr);
  int rc = LDG_OK;
  // every path destroys the events it created
  auto step = [&](hipError_t e) { if (!rc && e != hipSuccess) { ctx->err = hipGetErrorString(e); rc = LDG_EDEVICE; } };
  for (auto& e : ev) step(hipEventCreate(&e));
  for (int k = 0; k < iters && !rc; k++) {
    step(hipEventRecord(ev[2 * k], st));
    (variant ? ldg_k_demod_iso_cut : ldg_k_demod_iso)<<<n * MAX_BLOCKS_PER_READ, 1024, 0, st>>>(
          ctx->d_isomap, ctx->d_reads, ctx->cap, ctx->cap_first, ctx->cap_nsamp, ctx->cap_ring, ctx->fmt, ctx->tw, ctx->twk,
          ctx->rf_iso, ctx->fvideo, ctx->f05, ctx->iirtab, ctx->alf, ctx->arf, C,
          ctx->video, ctx->vread, ctx->vchan, ctx->d_status, ctx->d_ospill,
          ++ctx->park_epoch, ctx->d_stile, ctx->d_aslice, ctx->d_sst, ctx->d_sbits, ctx->d_bst, nullptr);
    step(hipEventRecord(ev[2 * k + 1], st));
  }
  if (!rc) rc = check_launch(ctx, variant ? "ldg_k_demod_iso_cut" : "ldg_k_demod_iso");
  if (!rc) step(hipStreamSynchronize(st));
  double tot = 0;
  for (int k = 0; k < iters && !rc; k++) {
    float ms = 0;
    step(hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
    tot += ms;
  }
  if (!rc) {
    *ms_per_launch = tot / iters;
    step(hipMemcpy(st_h.data(), ctx->d_status, st_h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < n && !rc; i++)
      if (st_h[slots[i]] == FS_EOF) { ctx->err = "demod_isolated: a read returned FS_EOF"; rc = LDG_ESTATE; }
  }
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  return rc;
}

int ldg_demod_isolated(ldg_ctx* ctx, int n, const int32_t* slots, int iters, double* ms_per_launch) {
  return ldg_demod_isolated_ex(ctx, n, slots, iters, 0, ms_per_launch);
}

int ldg_sync(ldg_ctx* ctx) {
  if (!ctx) return LDG_EINVAL;
  LDG_TRY(hipSetDevice(ctx->device));
  for (hipStream_t st : {ctx->stream2, ctx->scomb, ctx->stream, ctx->stream_b, ctx->sa, ctx->sout, ctx->srec, ctx->sprep}) LDG_TRY(hipStreamSynchronize(st));
  for (int k = 0; k < ctx->nsub; k++) LDG_TRY(hipStreamSynchronize(ctx->sub[k]));
  ctx->comb_pending = false;
  ctx->out_head = ctx->out_n = 0;
  prof_collect(ctx);
  return LDG_OK;
}

int ldg_comb_async(ldg_ctx* ctx, int n) {
  if (!ctx || n < 0 || n > ctx->max_frames) return LDG_EINVAL;
  if (!ctx->have_filters) { ctx->err = "comb: set the filters (the system) first"; return LDG_ESTATE; }
  if (n == 0) return LDG_OK;
  if (ctx->C.system == 0) return ldg_comb_ntsc_async(ctx, n);
  LDG_TRY(hipSetDevice(ctx->device));
  if (int rc = pal_alloc(ctx)) return rc;
  hipStream_t c = ctx->scomb;
  const int b = ctx->fb;
  LDG_TRY(hipStreamWaitEvent(c, ctx->ev_frames, 0));
  if (int rc = pal_launch(ctx, c, ctx->frame_buf(b), n)) return rc;
  LDG_TRY(hipEventRecord(ctx->ev_fbuf[b], c));
  ctx->fbuf_recorded[b] = true;
  ctx->comb_pending = true;
  return LDG_OK;
}

int ldg_comb_ntsc_async(ldg_ctx* ctx, int n) {
  if (!ctx || n < 0 || n > ctx->max_frames) return LDG_EINVAL;
  if (ctx->have_filters && ctx->C.system != 0) { ctx->err = "comb: NTSC only"; return LDG_EINVAL; }
  if (n == 0) return LDG_OK;
  LDG_TRY(hipSetDevice(ctx->device));
  if (int rc = comb_alloc(ctx)) return rc;
  // the comb of the frames just assembled, on its own stream (after that assembly);
  // the assembly after next, which rewrites this buffer, waits for ev_fbuf
  hipStream_t c = ctx->scomb;
  const int b = ctx->fb;
  LDG_TRY(hipStreamWaitEvent(c, ctx->ev_frames, 0));
  if (int rc = comb_launch(ctx, c, ctx->frame_buf(b), n, ctx->comb_rgb)) return rc;
  LDG_TRY(hipEventRecord(ctx->ev_fbuf[b], c));
  ctx->fbuf_recorded[b] = true;
  ctx->comb_pending = true;
  return LDG_OK;
}

int ldg_comb_ntsc(ldg_ctx* ctx, int n, const uint16_t* frames, uint16_t* rgb_out, int io_is_device) {
  if (!ctx || n < 0) return LDG_EINVAL;
  if (ctx->have_filters && ctx->C.system != 0) { ctx->err = "comb: NTSC only"; return LDG_EINVAL; }
  if (n == 0) return LDG_OK;
  if (!io_is_device && (!frames || !rgb_out)) return LDG_EINVAL;
  LDG_TRY(hipSetDevice(ctx->device));
  if (int rc = comb_alloc(ctx)) return rc;
  if (int rc = comb_quiesce(ctx)) return rc;
  hipStream_t s = ctx->stream2;
  const size_t fin = (size_t)comb::IN_X * comb::IN_Y, fout = (size_t)ctx->comb_opt.out_w() * ctx->comb_opt.out_rows * 3;
  for (int done = 0; done < n;) {
    const int m = (n - done) < ctx->max_frames ? (n - done) : ctx->max_frames;
    const uint16_t* src;
    uint16_t* dst;
    if (io_is_device) {
      src = (frames ? frames : ctx->frame_buf(ctx->fb)) + (size_t)done * fin;
      dst = rgb_out ? rgb_out + (size_t)done * fout : ctx->comb_rgb;
    } else {
      LDG_TRY(hipMemcpyAsync(ctx->comb_in, frames + (size_t)done * fin, m * fin * sizeof(uint16_t),
                             hipMemcpyHostToDevice, s));
      src = ctx->comb_in;
      dst = ctx->comb_rgb;
    }
    if (int rc = comb_launch(ctx, s, src, m, dst)) return rc;
    if (!io_is_device)
      LDG_TRY(hipMemcpyAsync(rgb_out + (size_t)done * fout, dst, m * fout * sizeof(uint16_t), hipMemcpyDeviceToHost,
                             s));
    done += m;
  }
  LDG_TRY(hipStreamSynchronize(s));
  prof_collect(ctx);
  return LDG_OK;
}

// ---- 3D comb with optical flow (comb-ntsc -d 3): the flow path of Process for one new
// input frame (comb-ntsc.cxx:851-858, OpticalFlow3D :600-662), BUILD-DEFINED (flow.hip).
// The frame's 2D split and luma fields, their pyramid and polynomial expansions; from the
// comb's third frame on the Farneback flow against the previous frame's expansions (the
// last flow as the initial estimate from the fourth on) and the weight map of the
// previous frame (window slot - 1).  Sequential: each flow starts from the last one.
static const int kFlowW[3] = {flow::FC, flow::FC / 2, flow::FC / 4};
static const int kFlowH[3] = {flow::FR, flow::FR / 2, (flow::FR + 3) / 4};   // 252, 126, 63 (cvRound)

static int flow_alloc(ldg_ctx* ctx) {
  auto& F = ctx->of;
  if (F.ybuf) return LDG_OK;
  const size_t px = (size_t)2 * flow::FR * flow::FC;
  int rc = 0;
  rc |= dmalloc(ctx, &F.ybuf, px);
  rc |= dmalloc(ctx, &F.t1, px);
  rc |= dmalloc(ctx, &F.t2, px);
  rc |= dmalloc(ctx, &F.I, px);
  rc |= dmalloc(ctx, &F.rows3, px * 3);
  rc |= dmalloc(ctx, &F.M, px * 5);
  rc |= dmalloc(ctx, &F.V, px * 5);
  for (int k = 0; k < 3; k++) {
    const size_t lp = (size_t)2 * kFlowH[k] * kFlowW[k];
    rc |= dmalloc(ctx, &F.R[0][k], lp * 5);
    rc |= dmalloc(ctx, &F.R[1][k], lp * 5);
    rc |= dmalloc(ctx, &F.fl[k], lp * 2);
  }
  rc |= dmalloc(ctx, &F.cv2d, (size_t)comb::ROWS_MAX * comb::CV_STRIDE);
  rc |= dmalloc(ctx, &F.kmap, (2 + (size_t)ctx->max_frames) * flow::FR * flow::FC);
  return rc ? LDG_ENOMEM : LDG_OK;
}

// getGaussianKernel (fixed tables for ksize <= 7 and sigma <= 0; oracle/farneback.py)
static flow::BlurK flow_blur_kernel(int ks, double sigma) {
  flow::BlurK K{};
  K.ks = ks;
  if (ks == 3 && sigma <= 0) {
    K.k[0] = 0.25; K.k[1] = 0.5; K.k[2] = 0.25;
    return K;
  }
  const double sg = sigma > 0 ? sigma : ((ks - 1) * 0.5 - 1) * 0.3 + 0.8;
  const double s2 = -0.5 / (sg * sg);
  double sum = 0;
  for (int i = 0; i < ks; i++) {
    const double x = i - (ks - 1) * 0.5;
    K.k[i] = std::exp(s2 * x * x);
    sum += K.k[i];
  }
  for (int i = 0; i < ks; i++) K.k[i] /= sum;
  return K;
}

// FarnebackPrepareGaussian(7, 1.5) (oracle/farneback.py prepare_gaussian)
static flow::PolyK flow_poly_kernel() {
  flow::PolyK P{};
  constexpr int n = flow::POLY_N;
  const double sigma = 1.5;
  double g[2 * n + 1], sum = 0;
  for (int x = -n; x <= n; x++) { g[x + n] = std::exp(-x * x / (2 * sigma * sigma)); sum += g[x + n]; }
  for (int x = -n; x <= n; x++) {
    P.g[x + n] = g[x + n] / sum;
    P.xg[x + n] = x * P.g[x + n];
    P.xxg[x + n] = (double)x * x * P.g[x + n];
  }
  double G[6][6] = {};
  for (int y = -n; y <= n; y++)
    for (int x = -n; x <= n; x++) {
      const double w = P.g[y + n] * P.g[x + n];
      G[0][0] += w;
      G[1][1] += w * x * x;
      G[3][3] += w * x * x * x * x;
      G[5][5] += w * x * x * y * y;
    }
  G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
  G[4][4] = G[3][3];
  G[3][4] = G[4][3] = G[5][5];
  // inverse by Gauss-Jordan with partial pivoting
  double A[6][12] = {};
  for (int i = 0; i < 6; i++) {
    for (int j = 0; j < 6; j++) A[i][j] = G[i][j];
    A[i][6 + i] = 1.0;
  }
  for (int c = 0; c < 6; c++) {
    int piv = c;
    for (int r = c + 1; r < 6; r++)
      if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
    for (int j = 0; j < 12; j++) std::swap(A[c][j], A[piv][j]);
    const double d = A[c][c];
    for (int j = 0; j < 12; j++) A[c][j] /= d;
    for (int r = 0; r < 6; r++)
      if (r != c) {
        const double f = A[r][c];
        for (int j = 0; j < 12; j++) A[r][j] -= f * A[c][j];
      }
  }
  P.ig11 = A[1][6 + 1];
  P.ig03 = A[0][6 + 3];
  P.ig33 = A[3][6 + 3];
  P.ig55 = A[5][6 + 5];
  return P;
}

static int flow_frame(ldg_ctx* ctx, hipStream_t st, const uint16_t* fr, int slot, double core, double range) {
  auto& F = ctx->of;
  const int64_t g = F.frames++;
  if (g == 0) return LDG_OK;                           // Process runs the flow path from framecount 1
  comb::CombOpt O2 = ctx->comb_opt;                    // the frame's 2D split, every line to 524
  O2.nrows = comb::IN_Y - O2.firstline;
  O2.bw = 0;
  LDG_LAUNCH_ON(st, "flow_split", ldg_k_comb_split_opt, O2.nrows, 256, fr, F.cv2d, O2);
  const double nry = ctx->comb_opt.nr_y < 4 ? 4 : ctx->comb_opt.nr_y;   // DoYNR(0, tbuf, 4)
  LDG_LAUNCH_ON(st, "flow_luma", ldg_k_flow_luma, 2 * flow::FR, 256, fr, F.cv2d, O2.firstline, nry, F.ybuf);
  // pyramid + expansions of the new frame (OpenCV's loop does both images each level; the
  // previous frame's are kept from its own turn -- the same values)
  static const flow::PolyK P = flow_poly_kernel();
  const int cur = F.rcur, prev = F.rcur ^ 1;
  for (int k = 0; k < 3; k++) {
    const double scale = std::ldexp(1.0, -k);
    const double sigma = (1.0 / scale - 1) * 0.5;
    int ks = ((int)std::nearbyint(sigma * 5)) | 1;
    if (ks < 3) ks = 3;
    const flow::BlurK K = flow_blur_kernel(ks, sigma);
    LDG_LAUNCH_ON(st, "flow_blur", ldg_k_flow_blur_rows, 2 * flow::FR, 256, F.ybuf, F.t1, K);
    LDG_LAUNCH_ON(st, "flow_blur", ldg_k_flow_blur_cols, 2 * flow::FR, 256, F.t1, F.t2, K);
    const int h = kFlowH[k], w = kFlowW[k];
    const double* I = F.t2;
    if (k) {
      LDG_LAUNCH_ON(st, "flow_resize", ldg_k_flow_resize, 2 * h, 256, F.t2, flow::FR, flow::FC, F.I, h, w, 1, 1.0);
      I = F.I;
    }
    LDG_LAUNCH_ON(st, "flow_poly", ldg_k_flow_poly_v, 2 * h, 256, I, h, w, F.rows3, P);
    LDG_LAUNCH_ON(st, "flow_poly", ldg_k_flow_poly_h, 2 * h, 256, F.rows3, h, w, F.R[cur][k], P);
  }
  if (g >= 2) {
    for (int k = 2; k >= 0; k--) {
      const int h = kFlowH[k], w = kFlowW[k];
      if (k == 2) {
        if (g >= 3)   // OPTFLOW_USE_INITIAL_FLOW: the last flow, area-resized, times the scale
          LDG_LAUNCH_ON(st, "flow_init", ldg_k_flow_area, 2 * h, 256, F.fl[0], kFlowH[0], kFlowW[0], F.fl[2], h, w,
                        0.25);
        else
          LDG_TRY(hipMemsetAsync(F.fl[2], 0, (size_t)2 * h * w * 2 * sizeof(double), st));
      } else {
        LDG_LAUNCH_ON(st, "flow_init", ldg_k_flow_resize, 2 * h, 256, F.fl[k + 1], kFlowH[k + 1], kFlowW[k + 1],
                      F.fl[k], h, w, 2, 2.0);
      }
      LDG_LAUNCH_ON(st, "flow_update", ldg_k_flow_update, 2 * h, 256, F.R[cur][k], F.R[prev][k], F.fl[k], h, w, F.M);
      for (int it = 0; it < flow::ITERS; it++) {
        LDG_LAUNCH_ON(st, "flow_blur_solve", ldg_k_flow_vsum, (2 * w * 5 + 255) / 256, 256, F.M, h, w, F.V);
        LDG_LAUNCH_ON(st, "flow_blur_solve", ldg_k_flow_hsum_solve, (2 * h + 63) / 64, 64, F.V, h, w, F.fl[k]);
        if (it < flow::ITERS - 1)
          LDG_LAUNCH_ON(st, "flow_update", ldg_k_flow_update, 2 * h, 256, F.R[cur][k], F.R[prev][k], F.fl[k], h, w,
                        F.M);
      }
    }
    F.klast = slot - 1;
    LDG_LAUNCH_ON(st, "flow_combk", ldg_k_flow_combk, flow::FR, 256, F.fl[0], core, range,
                  F.kmap + (size_t)F.klast * flow::FR * flow::FC);
  }
  F.rcur ^= 1;
  return check_launch(ctx, "flow kernels");
}

int ldg_comb_ntsc3d(ldg_ctx* ctx, int n, const uint16_t* frames, uint16_t* rgb_out, int* n_out, double core_ire,
                    double range_ire) {
  if (!ctx || n < 0 || !n_out || (n && (!frames || !rgb_out))) return LDG_EINVAL;
  *n_out = 0;
  if (ctx->have_filters && ctx->C.system != 0) { ctx->err = "comb: NTSC only"; return LDG_EINVAL; }
  // comb-ntsc main(): p_3dcore / p_3drange default 0 / 0.5 IRE with optical flow, 1.25 / 5.5 with -F,
  // then times irescale (:1074-1082; with flow they scale a motion in pixels, so the flow's
  // weight stays near 1 unless -c / -r are given)
  const bool of = ctx->comb_opt.of != 0;
  const double core = (core_ire < 0 ? (of ? 0.0 : 1.25) : core_ire) * comb::IRESCALE;
  const double range = (range_ire < 0 ? (of ? 0.5 : 5.5) : range_ire) * comb::IRESCALE;
  if (range == 0) { ctx->err = "comb 3D: range must be non-zero"; return LDG_EINVAL; }
  if (n == 0) return LDG_OK;
  LDG_TRY(hipSetDevice(ctx->device));
  if (int rc = comb_alloc(ctx)) return rc;
  const size_t fin = (size_t)comb::IN_X * comb::IN_Y, fout = (size_t)ctx->comb_opt.out_w() * ctx->comb_opt.out_rows * 3;
  if (!ctx->comb3_win && dmalloc(ctx, &ctx->comb3_win, (2 + (size_t)ctx->max_frames) * fin)) return LDG_ENOMEM;
  if (int rc = comb_quiesce(ctx)) return rc;
  if (of) {
    if (int rc = flow_alloc(ctx)) return rc;
  }
  hipStream_t s = ctx->stream2;
  int out = 0;
  for (int done = 0; done < n;) {
    const int m = (n - done) < ctx->max_frames ? (n - done) : ctx->max_frames;
    const int h = ctx->comb3_hist;                     // window slots [2 - h, 2): held inputs
    LDG_TRY(hipMemcpyAsync(ctx->comb3_win + 2 * fin, frames + (size_t)done * fin, m * fin * sizeof(uint16_t),
                           hipMemcpyHostToDevice, s));
    if (of) {
      // the flow path of each new frame, in order: the weight map of the frame before it
      for (int j = 0; j < m; j++)
        if (int rc = flow_frame(ctx, s, ctx->comb3_win + (size_t)(2 + j) * fin, 2 + j, core, range)) return rc;
    }
    const int c = m + h - 2;                           // frames that now have both neighbours
    if (c > 0) {
      const double* km = of ? ctx->of.kmap + (size_t)(3 - h) * flow::FR * flow::FC : nullptr;
      if (int rc = comb_launch(ctx, s, ctx->comb3_win + (size_t)(3 - h) * fin, c, ctx->comb_rgb, true, core, range,
                               km))
        return rc;
      LDG_TRY(hipMemcpyAsync(rgb_out + (size_t)out * fout, ctx->comb_rgb, c * fout * sizeof(uint16_t),
                             hipMemcpyDeviceToHost, s));
      out += c;
    }
    // hold the last two inputs in slots 0, 1 (copies in this order never overlap a later source)
    const int keep = (m + h) < 2 ? (m + h) : 2;
    for (int i = 0; i < keep; i++) {
      const int src = 2 + m - keep + i, dst = 2 - keep + i;
      if (src != dst)
        LDG_TRY(hipMemcpyAsync(ctx->comb3_win + (size_t)dst * fin, ctx->comb3_win + (size_t)src * fin,
                               fin * sizeof(uint16_t), hipMemcpyDeviceToDevice, s));
    }
    ctx->comb3_hist = keep;
    done += m;
  }
  LDG_TRY(hipStreamSynchronize(s));
  prof_collect(ctx);
  *n_out = out;
  return LDG_OK;
}

static int pal_alloc(ldg_ctx* ctx) {
  const size_t F = (size_t)ctx->max_frames;
  const size_t fin = (size_t)pal::IN_X * pal::IN_Y, fout = (size_t)pal::OUT_W * pal::OUT_H * 3;
  if (!ctx->pal_state) {
    int rc = 0;
    rc |= dmalloc(ctx, &ctx->pal_in, F * fin);
    rc |= dmalloc(ctx, &ctx->pal_rgb, F * fout);
    rc |= dmalloc(ctx, &ctx->pal_cv, F * pal::CV_ROWS * pal::CV_STRIDE);
    rc |= dmalloc(ctx, &ctx->pal_angle, F * pal::IN_Y);
    rc |= dmalloc(ctx, &ctx->pal_abl, F * pal::ABL_LINES);
    rc |= dmalloc(ctx, &ctx->pal_phase, F);
    rc |= dmalloc(ctx, &ctx->pal_state, 2);
    if (rc) return LDG_ENOMEM;
    const double init2[2] = {-1.0, -1.0};
    LDG_TRY(hipMemcpy(ctx->pal_state, init2, sizeof(init2), hipMemcpyHostToDevice));
    ctx->pal_scur = 0;
  }
  return LDG_OK;
}

// the PAL Y/C decoder's kernels over m <= max_frames device frames at `src` into pal_rgb
static int pal_launch(ldg_ctx* ctx, hipStream_t s, const uint16_t* src, int m) {
  if (m <= 0) return LDG_OK;
  const int cur = ctx->pal_scur;
  LDG_LAUNCH_ON(s, "pal_split", ldg_k_pal_split, m * pal::CV_ROWS, 256, src, ctx->pal_cv);
  LDG_LAUNCH_ON(s, "pal_angle", ldg_k_pal_angle, m, 256, ctx->pal_cv, m, ctx->pal_angle, ctx->pal_phase,
                ctx->pal_state + cur, ctx->pal_state + (cur ^ 1), ctx->pal_abl);
  ctx->pal_scur = cur ^ 1;
  LDG_LAUNCH_ON(s, "pal_out", ldg_k_pal_out, m * pal::OUT_H, 256, src, ctx->pal_cv, ctx->pal_angle,
                ctx->pal_phase, ctx->pal_abl, ctx->pal_rgb);
  ctx->pal_last_m = m;
  return check_launch(ctx, "pal comb kernels");
}

int ldg_comb_pal(ldg_ctx* ctx, int n, const uint16_t* frames, uint16_t* rgb_out) {
  if (!ctx || n < 0 || (n && (!frames || !rgb_out))) return LDG_EINVAL;
  if (n == 0) return LDG_OK;
  LDG_TRY(hipSetDevice(ctx->device));
  const size_t fin = (size_t)pal::IN_X * pal::IN_Y, fout = (size_t)pal::OUT_W * pal::OUT_H * 3;
  if (int rc = pal_alloc(ctx)) return rc;
  if (int rc = comb_quiesce(ctx)) return rc;
  hipStream_t s = ctx->stream2;
  for (int done = 0; done < n;) {
    const int m = (n - done) < ctx->max_frames ? (n - done) : ctx->max_frames;
    LDG_TRY(hipMemcpyAsync(ctx->pal_in, frames + (size_t)done * fin, m * fin * sizeof(uint16_t),
                           hipMemcpyHostToDevice, s));
    if (int rc = pal_launch(ctx, s, ctx->pal_in, m)) return rc;
    LDG_TRY(hipMemcpyAsync(rgb_out + (size_t)done * fout, ctx->pal_rgb, m * fout * sizeof(uint16_t),
                           hipMemcpyDeviceToHost, s));
    done += m;
  }
  LDG_TRY(hipStreamSynchronize(s));
  prof_collect(ctx);
  return LDG_OK;
}

int64_t ldg_debug_read(ldg_ctx* ctx, int slot, int what, void* dst, int64_t cap) {
  if (ctx && dst && (what == 50 || what == 51)) {
    // the NTSC comb's burst-level EMA: 50 = the values of the last call's lines, 51 = the carried state
    if (!ctx->comb_state) return LDG_EINVAL;
    if (hipSetDevice(ctx->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return LDG_EDEVICE;
    int64_t bytes = what == 50 ? (int64_t)ctx->comb_last_lines * 8 : 8;
    if (bytes > cap) bytes = cap;
    if (hipMemcpy(dst, what == 50 ? ctx->comb_abl : ctx->comb_state, bytes, hipMemcpyDeviceToHost) != hipSuccess)
      return LDG_EDEVICE;
    return bytes;
  }
  if (ctx && dst && what >= 70 && what <= 75) {
    // the optical flow's buffers for the last frame that took the flow path (flow_frame): 70 its luma
    // fields, 71..73 its expansions at levels 0..2, 74 the level-0 flow, 75 the weight map that flow wrote
    const auto& F = ctx->of;
    if (!F.ybuf || F.frames < (what >= 74 ? 3 : 2)) return LDG_EINVAL;
    if (hipSetDevice(ctx->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return LDG_EDEVICE;
    const int64_t px = (int64_t)flow::FR * flow::FC;
    const void* src = nullptr;
    int64_t bytes = 0;
    if (what == 70) {
      src = F.ybuf;
      bytes = 2 * px * 2;
    } else if (what <= 73) {
      const int k = what - 71;
      src = F.R[F.rcur ^ 1][k];                // flow_frame flips rcur once the frame is done
      bytes = (int64_t)2 * kFlowH[k] * kFlowW[k] * 5 * 8;
    } else if (what == 74) {
      src = F.fl[0];
      bytes = 2 * px * 2 * 8;
    } else {
      src = F.kmap + (int64_t)F.klast * px;
      bytes = px * 8;
    }
    if (bytes > cap) bytes = cap;
    if (hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return LDG_EDEVICE;
    return bytes;
  }
  if (ctx && dst && what >= 80 && what <= 84) {
    // the PAL Y/C decoder's buffers for the m frames of the last pal_launch: 80 SplitIQ's signed chroma,
    // 81 the burst angles, 82 the V-switch phases, 83 the burst-level EMA per line; 84 the carried EMA state
    const int64_t m = ctx->pal_last_m;
    if (!ctx->pal_state || m <= 0) return LDG_EINVAL;
    if (hipSetDevice(ctx->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return LDG_EDEVICE;
    const void* src = nullptr;
    int64_t bytes = 0;
    if (what == 80) {
      src = ctx->pal_cv;
      bytes = m * pal::CV_ROWS * pal::CV_STRIDE * 8;
    } else if (what == 81) {
      src = ctx->pal_angle;
      bytes = m * pal::IN_Y * 8;
    } else if (what == 82) {
      src = ctx->pal_phase;
      bytes = m * 4;
    } else if (what == 83) {
      src = ctx->pal_abl;
      bytes = m * pal::ABL_LINES * 8;
    } else {
      src = ctx->pal_state + ctx->pal_scur;
      bytes = 8;
    }
    if (bytes > cap) bytes = cap;
    if (hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return LDG_EDEVICE;
    return bytes;
  }
  if (!ctx || !dst || slot < 0 || slot >= ctx->max_reads || !ctx->live[slot]) return LDG_EINVAL;
  if (hipSetDevice(ctx->device) != hipSuccess) return LDG_EDEVICE;
  const ReadDesc& r = ctx->h_reads[slot];
  const void* src = nullptr;
  int64_t bytes = 0;
  if (what >= 0 && what < 5) {
    if (what >= ctx->C.n_chan) return LDG_EINVAL;
    if (what == CH_SYNC || what == CH_BURST) {
      // stored compact (chan.hpp): expand into the channel's full-rate slot first
      const int64_t chunks = ((int64_t)r.n_out + 15) / 16;
      if (chunks > 0) {
        LDG_TRY(hipDeviceSynchronize());   // the read's demod may be on any decode stream
        LDG_LAUNCH_ON(ctx->stream, "chan_expand", ldg_k_chan_expand, (int)((chunks + 63) / 64), 64, ctx->d_sst,
                      ctx->d_sbits, ctx->d_bst, ctx->video, ctx->vread, ctx->vchan, ctx->C, slot, what,
                      (int64_t)r.n_out);
        if (int rc = check_launch(ctx, "ldg_k_chan_expand")) return rc;
        LDG_TRY(hipStreamSynchronize(ctx->stream));
      }
    }
    src = ctx->video + (int64_t)slot * ctx->vread + (int64_t)what * ctx->vchan;
    bytes = (int64_t)r.n_out * 8;
  } else if (what == 10 || what == 11) {
    src = ctx->audio2 + (int64_t)slot * ctx->a2read + (int64_t)(what - 10) * ctx->a2chan;
    bytes = (int64_t)r.n_audio2 * 8;
  } else if (what == 12 || what == 13) {
    src = ctx->audio1 + (int64_t)slot * ctx->a1read + (int64_t)(what - 12) * ctx->a1chan;
    bytes = (int64_t)r.n_audio * 8;
  } else if (what >= 20 && what <= 24) {
    const int arr[5] = {LL1, LL2, LL3, LL4, LLF};
    src = ctx->d_lines + (int64_t)slot * LINES_STRIDE + (int64_t)arr[what - 20] * MAX_LINES;
    bytes = (int64_t)MAX_LINES * 8;
  } else if (what == 30) {
    src = ctx->d_blevel + (int64_t)slot * MAX_LINES;
    bytes = (int64_t)MAX_LINES * 4;
  } else if (what == 31) {
    src = ctx->d_bad + (int64_t)slot * MAX_LINES;
    bytes = MAX_LINES;
  } else if (what == 40) {
    src = ctx->d_pic + (int64_t)slot * ctx->pic_stride;
    bytes = ctx->pic_stride * 2;
  } else if (what == 41) {
    src = ctx->d_peaks + (int64_t)slot * MAX_PEAKS;
    bytes = (int64_t)MAX_PEAKS * 4;
  } else if (what == 60 || what == 61) {
    // the slot's dropout runs / per-row counts as the last ldg_field_dropouts left them
    if (!ctx->d_drop_runs) return LDG_EINVAL;
    if (hipStreamSynchronize(ctx->sout) != hipSuccess) return LDG_EDEVICE;
    src = what == 60 ? (const void*)(ctx->d_drop_runs + (int64_t)slot * DROP_RUNS_STRIDE)
                     : (const void*)(ctx->d_drop_cnt + (int64_t)slot * MAX_LINES);
    bytes = what == 60 ? (int64_t)DROP_RUNS_STRIDE * 2 : (int64_t)MAX_LINES * 4;
  } else {
    return LDG_EINVAL;
  }
  if (bytes > cap) bytes = cap;
  if (hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return LDG_EDEVICE;
  return bytes;
}

int ldg_debug_rf_table(ldg_ctx* ctx, double mtf, double* dst) {
  // the demod's RF filter table for one MTF level (kernel ldg_k_rf_table, the one a
  // decode call builds per distinct level), returned in natural bin order
  if (!ctx || !dst || !ctx->rfvideo) return LDG_EINVAL;
  LDG_TRY(hipSetDevice(ctx->device));
  LDG_TRY(hipDeviceSynchronize());
  double* d_m = nullptr;
  double2* d_t = nullptr;
  LDG_TRY(hipMalloc(&d_m, sizeof(double)));
  if (hipMalloc(&d_t, sizeof(double2) * BLOCKLEN) != hipSuccess) {
    (void)hipFree(d_m);
    return LDG_ENOMEM;
  }
  std::vector<double2> tab(BLOCKLEN);
  int rc = LDG_OK;
  if (hipMemcpy(d_m, &mtf, sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = LDG_EDEVICE;
  if (rc == LDG_OK) {
    hipLaunchKernelGGL(ldg_k_rf_table, dim3(BLOCKLEN / 256, 1), dim3(256), 0, ctx->stream, ctx->rfvideo, ctx->mtf,
                         ctx->mtf_logabs, ctx->mtf_arg, d_m, d_t);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(tab.data(), d_t, sizeof(double2) * BLOCKLEN, hipMemcpyDeviceToHost) != hipSuccess)
      rc = LDG_EDEVICE;
  }
  (void)hipFree(d_m);
  (void)hipFree(d_t);
  if (rc != LDG_OK) return rc;
  for (int o = 0; o < BLOCKLEN; o++) {
    const int p = o & (HALF - 1);
    const int k = dr_nat(p) +
                  (o >= HALF ? HALF : 0);
    dst[2 * k] = tab[o].x;
    dst[2 * k + 1] = tab[o].y;
  }
  return LDG_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Synthetic capture generation (tooling; synth.hip).
extern "C" int ldg_synth_capture(ldg_ctx* ctx, const ldg_synth_params* p, const double* fir63, const double* emph,
                                 const uint32_t* codes, int64_t ncodeframes) {
  if (!ctx || !p || !fir63 || !emph || !codes || p->nsamples <= 0 || p->fmt < 0 || p->fmt > 3) return LDG_EINVAL;
  if (ctx->system != 0) { ctx->err = "synth: NTSC only"; return LDG_EINVAL; }
  LDG_TRY(hipSetDevice(ctx->device));
  if (int rc = ldg_stream_close(ctx)) return rc;
  ctx->cap_ring = 0;
  hipStream_t s = ctx->stream;
  SynthConst S{};
  S.H = 227.5 / (315.0 / 88.0);
  S.spl = 40e6 * S.H / 1e6;
  S.t0_lines = p->start_line;
  S.fsc = 315e6 / 88;
  S.ire0 = 8100000.0;
  S.hz_ire = 1700000 / 140.0;
  S.sync = -40.0;
  S.burst_ire = 20.0;
  S.b0 = emph[0]; S.b1 = emph[1]; S.a1 = emph[2];
  S.audio_l = (1000000 * 315.0 / 88 / 227.5) * 146.25;
  S.audio_r = (1000000 * 315.0 / 88 / 227.5) * 178.75;
  S.noise = p->noise;
  for (int k = 0; k < SY_FIR; k++) S.fir[k] = fir63[k];
  S.lines = 525;
  S.fmt = p->fmt;
  S.seed = p->seed;
  const int64_t n = p->nsamples;
  const int64_t nblk = (n + SY_CH - 1) / SY_CH;
  uint32_t* d_codes = nullptr;
  double* d_tot = nullptr;
  if (dmalloc(ctx, &d_codes, (size_t)ncodeframes * 3) || dmalloc(ctx, &d_tot, (size_t)nblk)) return LDG_ENOMEM;
  LDG_TRY(hipMemcpy(d_codes, codes, ncodeframes * 3 * sizeof(uint32_t), hipMemcpyHostToDevice));
  constexpr int64_t SY_LAUNCH = 1 << 22;     // chunks per launch: 2^30 work-items
  for (int64_t b0 = 0; b0 < nblk; b0 += SY_LAUNCH) {
    ldg_k_synth_pass1<<<(unsigned)std::min(SY_LAUNCH, nblk - b0), SY_T, 0, s>>>(S, d_codes, ncodeframes, d_tot, b0);
    if (int rc = check_launch(ctx, "ldg_k_synth_pass1")) return rc;
  }
  std::vector<double> tot(nblk);
  LDG_TRY(hipMemcpyAsync(tot.data(), d_tot, nblk * sizeof(double), hipMemcpyDeviceToHost, s));
  LDG_TRY(hipStreamSynchronize(s));
  const double TWO_PI = 6.283185307179586;
  double acc = 0.0;
  for (int64_t b = 0; b < nblk; b++) {
    const double t = tot[b];
    tot[b] = acc;
    acc = std::fmod(acc + std::fmod(t, TWO_PI), TWO_PI);
  }
  LDG_TRY(hipMemcpy(d_tot, tot.data(), nblk * sizeof(double), hipMemcpyHostToDevice));
  size_t nbytes;
  switch (p->fmt) {
    case 0: nbytes = (size_t)n; break;
    case 1: nbytes = (size_t)n * 2; break;
    case 2: nbytes = (size_t)((n + 2) / 3) * 4; break;
    default: nbytes = (size_t)((n + 3) / 4) * 5; break;
  }
  if (ctx->cap_owned) dfree(ctx->cap);
  ctx->cap = nullptr;
  ctx->cap_owned = false;
  if (dmalloc(ctx, &ctx->cap, nbytes + 64)) return LDG_ENOMEM;
  ctx->cap_owned = true;
  ctx->cap_alloc = nbytes;
  uint8_t* dst = ctx->cap;
  uint16_t* stage = nullptr;
  if (p->fmt >= 2) {
    const int64_t padn = ((n + 11) / 12) * 12;
    if (dmalloc(ctx, &stage, (size_t)padn)) return LDG_ENOMEM;
    LDG_TRY(hipMemsetAsync(stage, 0, padn * sizeof(uint16_t), s));
    dst = (uint8_t*)stage;
  }
  for (int64_t b0 = 0; b0 < nblk; b0 += SY_LAUNCH) {
    ldg_k_synth_pass2<<<(unsigned)std::min(SY_LAUNCH, nblk - b0), SY_T, 0, s>>>(S, d_codes, ncodeframes, d_tot, n, dst, b0);
    if (int rc = check_launch(ctx, "ldg_k_synth_pass2")) return rc;
  }
  if (p->fmt >= 2) {
    const int64_t ng = p->fmt == 2 ? (n + 2) / 3 : (n + 3) / 4;
    constexpr int64_t PK_LAUNCH = (int64_t)1 << 30;   // groups per launch
    for (int64_t g0 = 0; g0 < ng; g0 += PK_LAUNCH) {
      const int64_t m = std::min(PK_LAUNCH, ng - g0);
      ldg_k_synth_pack10<<<(unsigned)((m + 255) / 256), 256, 0, s>>>(stage, ng, p->fmt, ctx->cap, g0);
      if (int rc = check_launch(ctx, "ldg_k_synth_pack10")) return rc;
    }
  }
  LDG_TRY(hipStreamSynchronize(s));
  dfree(stage);
  dfree(d_codes);
  dfree(d_tot);
  ctx->fmt = p->fmt;
  ctx->cap_first = 0;
  ctx->cap_nsamp = n;
  return LDG_OK;
}

extern "C" int64_t ldg_capture_download(ldg_ctx* ctx, void* dst, int64_t offset, int64_t nbytes) {
  if (!ctx || !dst || offset < 0 || nbytes < 0 || !ctx->cap) return LDG_EINVAL;
  if (ctx->cs) return LDG_ESTATE;                   // a streamed capture has no resident copy
  if ((size_t)offset >= ctx->cap_alloc) return 0;
  if ((size_t)(offset + nbytes) > ctx->cap_alloc) nbytes = (int64_t)ctx->cap_alloc - offset;
  if (hipSetDevice(ctx->device) != hipSuccess) return LDG_EDEVICE;
  // hipMemcpyDefault: dst may be host memory or a device buffer (unified addressing)
  if (hipMemcpy(dst, ctx->cap + offset, nbytes, hipMemcpyDefault) != hipSuccess) return LDG_EDEVICE;
  return nbytes;
}

extern "C" int ldg_profile_enable(ldg_ctx* ctx, int on) {
  if (!ctx) return LDG_EINVAL;
  if (on) {
    LDG_TRY(hipSetDevice(ctx->device));
    if (!ctx->d_span && dmalloc(ctx, &ctx->d_span, 2 * (size_t)ldg_ctx::SPAN_MAX)) return LDG_ENOMEM;
    for (hipStream_t st : {ctx->stream, ctx->stream_b, ctx->stream2, ctx->scomb, ctx->sa, ctx->sout, ctx->srec, ctx->sprep})
      LDG_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < ctx->nsub; k++) LDG_TRY(hipStreamSynchronize(ctx->sub[k]));
    LDG_TRY(hipMemset(ctx->d_span, 0, 2 * (size_t)ldg_ctx::SPAN_MAX * sizeof(unsigned long long)));
    // host steady clock -> device constant-rate clock: a one-lane kernel reads the
    // device clock between two host reads; the tightest of five brackets is kept
    // (error <= half its width, a few microseconds)
    int64_t best = -1;
    for (int k = 0; k < 5; k++) {
      LDG_TRY(hipMemsetAsync(ctx->d_span, 0, sizeof(unsigned long long), ctx->stream));
      LDG_TRY(hipStreamSynchronize(ctx->stream));
      const int64_t h0 = steady_ns();
      hipLaunchKernelGGL(ldg_k_clock, dim3(1), dim3(64), 0, ctx->stream, ctx->d_span);
      LDG_TRY(hipStreamSynchronize(ctx->stream));
      const int64_t h1 = steady_ns();
      unsigned long long t = 0;
      LDG_TRY(hipMemcpy(&t, ctx->d_span, sizeof(t), hipMemcpyDeviceToHost));
      if (best < 0 || h1 - h0 < best) {
        best = h1 - h0;
        ctx->cal_ticks = t;
        ctx->cal_ns = h0 + (h1 - h0) / 2;
      }
    }
    LDG_TRY(hipMemset(ctx->d_span, 0, sizeof(unsigned long long)));
  }
  ctx->span_n = 0;
  ctx->span_issue_ns.clear();
  ctx->prof_on = on != 0;
  ctx->prof_only = on == 2 ? "demod" : nullptr;
  ctx->prof_pending.clear();
  ctx->prof_stats.clear();
  return LDG_OK;
}

// The demod launches' execution spans since ldg_profile_enable: their count and
// summed duration (first workgroup start to last workgroup end, in ms).
extern "C" int ldg_profile_spans(ldg_ctx* ctx, double* total_ms, int64_t* count) {
  if (!ctx || !total_ms || !count) return LDG_EINVAL;
  *total_ms = 0;
  *count = 0;
  if (!ctx->d_span || !ctx->span_n) return LDG_OK;
  LDG_TRY(hipSetDevice(ctx->device));
  LDG_TRY(hipStreamSynchronize(ctx->stream));
  LDG_TRY(hipStreamSynchronize(ctx->stream_b));
  int khz = 0;
  LDG_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
  if (khz <= 0) { ctx->err = "no wall-clock rate"; return LDG_EDEVICE; }
  std::vector<unsigned long long> h(2 * (size_t)ctx->span_n);
  LDG_TRY(hipMemcpy(h.data(), ctx->d_span, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  // LDG_SPANDUMP=<file>: every launch's span (ms from the first start) for timeline tools
  FILE* dump = getenv("LDG_SPANDUMP") ? fopen(getenv("LDG_SPANDUMP"), "w") : nullptr;
  const unsigned long long t0 = ~h[0];
  for (int i = 0; i < ctx->span_n; i++) {
    const unsigned long long st = ~h[2 * i], en = h[2 * i + 1];
    if (h[2 * i] == 0 || en == 0 || en < st) continue;   // launch without workgroups / not recorded
    *total_ms += (double)(en - st) / (double)khz;
    (*count)++;
    if (dump) fprintf(dump, "%.4f %.4f\n", (double)(long long)(st - t0) / khz, (double)(long long)(en - t0) / khz);
  }
  if (dump) fclose(dump);
  return LDG_OK;
}

// Every profiled demod launch in issue order: (start, end, host issue) in ms on the
// device's constant-rate clock, from the first launch's start (an issue time
// mapped through the calibration of ldg_profile_enable, a few microseconds
// uncertain), and the issue time on the host's steady clock in ms (CLOCK_MONOTONIC:
// Python's time.perf_counter() * 1e3, for host timelines).  Returns the launch
// count (at most max rows of four written), or < 0.
extern "C" int ldg_profile_span_table(ldg_ctx* ctx, double* out, int max) {
  if (!ctx || (max > 0 && !out)) return LDG_EINVAL;
  if (!ctx->d_span || !ctx->span_n) return 0;
  LDG_TRY(hipSetDevice(ctx->device));
  LDG_TRY(hipStreamSynchronize(ctx->stream));
  LDG_TRY(hipStreamSynchronize(ctx->stream_b));
  int khz = 0;
  LDG_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
  if (khz <= 0) { ctx->err = "no wall-clock rate"; return LDG_EDEVICE; }
  std::vector<unsigned long long> h(2 * (size_t)ctx->span_n);
  LDG_TRY(hipMemcpy(h.data(), ctx->d_span, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  const double t0 = (double)~h[0];
  int n = 0;
  for (int i = 0; i < ctx->span_n && n < max; i++, n++) {
    const unsigned long long st = ~h[2 * i], en = h[2 * i + 1];
    const bool ok = h[2 * i] != 0 && en != 0 && en >= st;
    const double iss = (double)ctx->cal_ticks + (double)(ctx->span_issue_ns[i] - ctx->cal_ns) * khz / 1e6;
    out[4 * n] = ok ? ((double)st - t0) / khz : NAN;
    out[4 * n + 1] = ok ? ((double)en - t0) / khz : NAN;
    out[4 * n + 2] = (iss - t0) / khz;
    out[4 * n + 3] = (double)ctx->span_issue_ns[i] / 1e6;
  }
  return n;
}

// The time during which at least one demod launch was executing (the union of
// the launch spans since ldg_profile_enable, in ms) and the launch count: with
// two demod streams consecutive launches overlap, so the summed spans count the
// shared time twice.
extern "C" int ldg_profile_spans_union(ldg_ctx* ctx, double* union_ms, int64_t* count) {
  if (!ctx || !union_ms || !count) return LDG_EINVAL;
  *union_ms = 0;
  *count = 0;
  if (!ctx->d_span || !ctx->span_n) return LDG_OK;
  LDG_TRY(hipSetDevice(ctx->device));
  LDG_TRY(hipStreamSynchronize(ctx->stream));
  LDG_TRY(hipStreamSynchronize(ctx->stream_b));
  int khz = 0;
  LDG_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
  if (khz <= 0) { ctx->err = "no wall-clock rate"; return LDG_EDEVICE; }
  std::vector<unsigned long long> h(2 * (size_t)ctx->span_n);
  LDG_TRY(hipMemcpy(h.data(), ctx->d_span, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::vector<std::pair<unsigned long long, unsigned long long>> iv;
  for (int i = 0; i < ctx->span_n; i++) {
    const unsigned long long st = ~h[2 * i], en = h[2 * i + 1];
    if (h[2 * i] == 0 || en == 0 || en < st) continue;
    iv.emplace_back(st, en);
  }
  std::sort(iv.begin(), iv.end());
  unsigned long long cs = 0, ce = 0, tot = 0;
  for (size_t i = 0; i < iv.size(); i++) {
    if (i == 0 || iv[i].first > ce) {
      tot += ce - cs;
      cs = iv[i].first;
      ce = iv[i].second;
    } else if (iv[i].second > ce) {
      ce = iv[i].second;
    }
  }
  tot += ce - cs;
  *union_ms = (double)tot / (double)khz;
  *count = (int64_t)iv.size();
  return LDG_OK;
}

extern "C" int ldg_profile_read(ldg_ctx* ctx, ldg_kernel_stat* out, int max) {
  if (!ctx || (max > 0 && !out)) return LDG_EINVAL;
  int i = 0;
  for (auto& kv : ctx->prof_stats) {
    if (i < max) {
      std::memset(out[i].name, 0, sizeof(out[i].name));
      std::strncpy(out[i].name, kv.first.c_str(), sizeof(out[i].name) - 1);
      out[i].launches = kv.second.first;
      out[i].total_ms = kv.second.second;
    }
    i++;
  }
  return i;
}

#ifdef LDG_STAMPS
// profiling builds: the demod's phase stamps ([LDG_STAMP_BLOCKS][32] shader clocks)
extern "C" int ldg_debug_stamps(unsigned long long* dst) {
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps), sizeof(g_stamps)) == hipSuccess ? LDG_OK : LDG_EDEVICE;
}
// [KST_KERNELS][KST_BLOCKS][KST_PHASES] shader clocks (common.hpp KSTAMP); clear: zero them first
extern "C" int ldg_debug_kstamps(unsigned long long* dst, int clear) {
  if (clear) {
    static unsigned long long zero[KST_KERNELS][KST_BLOCKS][KST_PHASES];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_kst), zero, sizeof(zero)) == hipSuccess ? LDG_OK : LDG_EDEVICE;
  }
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_kst), sizeof(g_kst)) == hipSuccess ? LDG_OK : LDG_EDEVICE;
}
#endif
