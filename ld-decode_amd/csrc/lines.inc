// Host side of the NTSC line services (lines.hip; build-defined, DESIGN.md section 7f):
// ldg_field_line_services and ldg_frames_line_services of include/ldgpu.h.  Unity-built after
// abi.inc, whose launch, staging and error helpers it uses.

struct ldg_lines_state {
  // a stream of its own: a call waits for its own kernel and copy only, not for the audio or
  // the frames queued on the context's output streams
  hipStream_t st = nullptr;
  // slot form: max_reads entries
  int32_t* d_map = nullptr;
  ldg::LineRec* d_rec = nullptr;
  // frames form: a chunk's staging, so a decode on this context never sees it
  uint16_t* d_frames = nullptr;      // LINES_CHUNK host frames
  ldg::LineRec* d_frec = nullptr;    // their 2 * LINES_CHUNK records
};

static void lines_free(ldg_ctx* ctx) {
  ldg_lines_state* S = ctx->lines;
  if (!S) return;
  if (S->st) {
    (void)hipStreamSynchronize(S->st);
    (void)hipStreamDestroy(S->st);
  }
  for (void* p : {(void*)S->d_map, (void*)S->d_rec, (void*)S->d_frames, (void*)S->d_frec}) dfree(p);
  delete S;
  ctx->lines = nullptr;
}

namespace {

constexpr int LINES_CHUNK = 32;                       // frames a launch of the frames form takes
constexpr size_t LINES_FRAME_PX = (size_t)ldg::LS_W * 525;

// what both calls refuse before touching the device; 0: go on, 1: nothing to do
int lines_args(ldg_ctx* ctx, const char* fn, int n, const void* in, const char* in_name, const void* out, int* rc) {
  auto bad = [&](const char* what) {
    ctx->err = std::string(fn) + ": " + what;
    *rc = LDG_EINVAL;
    return 1;
  };
  *rc = LDG_OK;
  if (ctx->system != LDG_SYSTEM_NTSC) return bad("the context is PAL; the line services are defined for NTSC only");
  if (n < 0) return bad("n must be >= 0");
  if (n == 0) return 1;
  if (!in) return bad((std::string(in_name) + " must not be NULL").c_str());
  if (!out) return bad("out must not be NULL");
  return 0;
}

int lines_state(ldg_ctx* ctx, ldg_lines_state** out) {
  if (!ctx->lines) ctx->lines = new (std::nothrow) ldg_lines_state();
  if (!ctx->lines) {
    ctx->err = "line services: out of memory";
    return LDG_ENOMEM;
  }
  ldg_lines_state* S = ctx->lines;
  if (!S->st && hipStreamCreateWithFlags(&S->st, hipStreamNonBlocking) != hipSuccess) {
    S->st = nullptr;
    ctx->err = "line services: hipStreamCreate failed";
    return LDG_EDEVICE;
  }
  *out = S;
  return LDG_OK;
}

}  // namespace

int ldg_field_line_services(ldg_ctx* ctx, int n, const int32_t* slots, ldg_line_services* out) {
  if (!ctx) return LDG_EINVAL;
  int rc;
  if (lines_args(ctx, "ldg_field_line_services", n, slots, "slots", out, &rc)) return rc;
  if (n > ctx->max_reads) {
    ctx->err = "ldg_field_line_services: n must be <= max_reads";
    return LDG_EINVAL;
  }
  for (int i = 0; i < n; i++)
    if (slots[i] < 0 || slots[i] >= ctx->max_reads || !ctx->live[slots[i]]) {
      ctx->err = "ldg_field_line_services: slots must name live slots of this context";
      return LDG_EINVAL;
    }
  LDG_TRY(hipSetDevice(ctx->device));
  ldg_lines_state* S;
  if ((rc = lines_state(ctx, &S))) return rc;
  if (!S->d_rec) {
    if ((rc = dmalloc(ctx, &S->d_map, (size_t)ctx->max_reads))) return rc;
    if ((rc = dmalloc(ctx, &S->d_rec, (size_t)ctx->max_reads))) return rc;
  }
  hipStream_t s = S->st;         // the slots are live: their .tbc lines are complete and stay until reused
  if ((rc = stage_h2d(ctx, S->d_map, slots, n * sizeof(int32_t), s))) return rc;
  LDG_LAUNCH_ON(s, "line_services", ldg_k_line_services, dim3(ldg::LS_SERVICES, (unsigned)n), 64, ctx->d_pic,
                ctx->pic_stride, S->d_map, ctx->d_recs, S->d_rec);
  if ((rc = check_launch(ctx, "ldg_k_line_services"))) return rc;
  LDG_TRY(hipMemcpyAsync(out, S->d_rec, (size_t)n * sizeof(ldg_line_services), hipMemcpyDeviceToHost, s));
  LDG_TRY(hipStreamSynchronize(s));
  prof_collect(ctx);
  return LDG_OK;
}

int ldg_frames_line_services(ldg_ctx* ctx, int n, const uint16_t* frames, int frames_is_device,
                             ldg_line_services* out) {
  if (!ctx) return LDG_EINVAL;
  int rc;
  if (lines_args(ctx, "ldg_frames_line_services", n, frames, "frames", out, &rc)) return rc;
  LDG_TRY(hipSetDevice(ctx->device));
  ldg_lines_state* S;
  if ((rc = lines_state(ctx, &S))) return rc;
  if (!S->d_frec && (rc = dmalloc(ctx, &S->d_frec, (size_t)2 * LINES_CHUNK))) return rc;
  if (!frames_is_device && !S->d_frames && (rc = dmalloc(ctx, &S->d_frames, LINES_CHUNK * LINES_FRAME_PX))) return rc;
  hipStream_t st = S->st;
  for (int done = 0; done < n;) {
    const int m = (n - done) < LINES_CHUNK ? (n - done) : LINES_CHUNK;
    const uint16_t* src = frames + (size_t)done * LINES_FRAME_PX;
    if (!frames_is_device) {
      LDG_TRY(hipMemcpyAsync(S->d_frames, src, (size_t)m * LINES_FRAME_PX * sizeof(uint16_t), hipMemcpyHostToDevice, st));
      src = S->d_frames;
    }
    LDG_LAUNCH_ON(st, "line_services", ldg_k_line_services, dim3(ldg::LS_SERVICES, (unsigned)(2 * m)), 64, src,
                  (int64_t)LINES_FRAME_PX, (const int32_t*)nullptr, (const FieldRec*)nullptr, S->d_frec);
    if ((rc = check_launch(ctx, "ldg_k_line_services"))) return rc;
    LDG_TRY(hipMemcpyAsync(out + (size_t)2 * done, S->d_frec, (size_t)2 * m * sizeof(ldg_line_services),
                           hipMemcpyDeviceToHost, st));
    LDG_TRY(hipStreamSynchronize(st));
    done += m;
  }
  prof_collect(ctx);
  return LDG_OK;
}
