// C ABI of libdctae.so: context, options, timing, plan upload and workspace.
// See include/dctae.h for the contract of every entry point; dctae_ctx.h
// lists the host units.
#include "dctae_ctx.h"
#include "../../include/dctae_u8.h"
#include "../../include/dctae_u8_out.h"

using namespace dctae;

thread_local std::string dctae::g_err;

namespace {

// reference colour constants (util.py:21-43), built exactly like the
// reference does in fp32: Trgb2lms = MHPE @ MsRGB; Tlms2rgb = inverse; Mipt^-1.
// The Python layer overrides these with torch-computed bits (ctx->cm) so the
// matrix inverses carry the reference's exact fp32 values.
void default_colors(ColorMats& cm) {
  const double srgb[9] = {0.4124564, 0.3575761, 0.1804375, 0.2126729, 0.7151522, 0.0721750,
                          0.0193339, 0.1191920, 0.9503041};
  const double hpe[9] = {0.4002, 0.7076, -0.0807, -0.2280, 1.1500, 0.0612, 0, 0, 0.9184};
  const double ipt[9] = {0.4, 0.4, 0.2, 4.455, -4.851, 0.3960, 0.8056, 0.3572, -1.1628};
  double m[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0;
      for (int k = 0; k < 3; ++k) s += (double)(float)hpe[3 * i + k] * (double)(float)srgb[3 * k + j];
      m[3 * i + j] = s;
    }
  auto inv3 = [](const double* a, double* o) {
    double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) +
                 a[2] * (a[3] * a[7] - a[4] * a[6]);
    o[0] = (a[4] * a[8] - a[5] * a[7]) / det;
    o[1] = (a[2] * a[7] - a[1] * a[8]) / det;
    o[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    o[3] = (a[5] * a[6] - a[3] * a[8]) / det;
    o[4] = (a[0] * a[8] - a[2] * a[6]) / det;
    o[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    o[6] = (a[3] * a[7] - a[4] * a[6]) / det;
    o[7] = (a[1] * a[6] - a[0] * a[7]) / det;
    o[8] = (a[0] * a[4] - a[1] * a[3]) / det;
  };
  double mi[9], ii[9], ipd[9];
  for (int i = 0; i < 9; ++i) ipd[i] = (float)ipt[i];
  inv3(m, mi);
  inv3(ipd, ii);
  for (int i = 0; i < 9; ++i) {
    cm.rgb2lms[i] = (float)m[i];
    cm.lms2rgb[i] = (float)mi[i];
    cm.lms2ipt[i] = (float)ipt[i];
    cm.ipt2lms[i] = (float)ii[i];
  }
}

// the call-ordering event (OrderedCall) only orders this context's calls
// across streams of one device: no system-scope fence (its cache write-back
// sat between back-to-back calls)
constexpr unsigned kDoneEvtFlags = hipEventDisableTiming | hipEventDisableSystemFence;

constexpr const char* kScratchName[kNumScratch] = {"workspace", "staging", "PatchNorm statistics scratch",
                                                   "VectorQuantize scratch", "LFQ projection scratch"};

}  // namespace

int OrderedCall::upload(const PlanBuf& pb, uint8_t** base, uint64_t plan_id) {
  const size_t n = pb.bytes.size();
  *base = ctx->plan.p;
  if (n == 0) return 0;
  if (plan_id != 0 && plan_id == ctx->plan_last_id) return 0;
  if (n == ctx->plan_last.size() && std::memcmp(pb.bytes.data(), ctx->plan_last.data(), n) == 0) {
    ctx->plan_last_id = plan_id;
    return 0;
  }
  if (n > ctx->plan.cap) {
    // both copies go and come back together; a failure leaves no device copy and nothing cached
    const size_t cap = std::max<size_t>(n * 2, 1 << 20);
    ctx->plan_last.clear();
    ctx->plan_last_id = 0;
    HIPCHK(ctx, hipDeviceSynchronize());   // no upload still reads plan_host
    if (ctx->plan_host) hipHostFree(ctx->plan_host);
    ctx->plan_host = nullptr;
    ctx->plan.release();
    HIPCHK(ctx, hipHostMalloc((void**)&ctx->plan_host, cap, hipHostMallocDefault));
    if (int rc = ctx->plan.grow(ctx, cap, "plan")) return rc;
    *base = ctx->plan.p;
  } else {
    HIPCHK(ctx, hipEventSynchronize(ctx->plan_evt));  // previous upload finished reading plan_host
  }
  std::memcpy(ctx->plan_host, pb.bytes.data(), n);
  HIPCHK(ctx, hipMemcpyAsync(ctx->plan.p, ctx->plan_host, n, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipEventRecord(ctx->plan_evt, s));
  ctx->plan_last = pb.bytes;
  ctx->plan_last_id = plan_id;
  return 0;
}

int OrderedCall::scratch_bytes(Scratch which, size_t bytes, uint8_t** out) {
  DevBuf& b = ctx->scratch[which];
  const bool grew = bytes > b.cap;
  if (int rc = b.grow(ctx, bytes, kScratchName[which])) return rc;
  *out = b.p;
  // ws_poison: each of the five buffers is filled when this call first asks
  // for it (and when it grows it), never over what it wrote since
  if (ctx->opt.ws_poison && b.p && (grew || !(poisoned & (1u << which)))) {
    poisoned |= 1u << which;
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemset(b.p, 0xff, b.cap));
    HIPCHK(ctx, hipDeviceSynchronize());
  }
  return 0;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" {

int dctae_abi_version(void) { return DCTAE_ABI_VERSION; }

int dctae_ctx_create(int device, dctae_ctx** out) {
  if (!out) return DCTAE_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    g_err = "no HIP device";
    return DCTAE_EHIP;
  }
  if (device < 0 || device >= n) {
    g_err = "bad device index";
    return DCTAE_EINVAL;
  }
  if (hipSetDevice(device) != hipSuccess) {
    g_err = "hipSetDevice failed";
    return DCTAE_EHIP;
  }
  dctae_ctx* c = new dctae_ctx();
  c->device = device;
  default_colors(c->cm);
  if (hipEventCreateWithFlags(&c->plan_evt, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->done_evt, kDoneEvtFlags) != hipSuccess ||
      hipMalloc((void**)&c->err_dev, sizeof(int)) != hipSuccess || hipMemset(c->err_dev, 0, sizeof(int)) != hipSuccess) {
    g_err = "context allocation failed";
    delete c;
    return DCTAE_EHIP;
  }
  c->fft_tab_cap = 1 << 20;
  {
    const char* e = getenv("DCTAE_WS_POISON");
    c->opt.ws_poison = e && e[0] == '1';
  }
  if (hipMalloc((void**)&c->fft_tab, c->fft_tab_cap * sizeof(float2)) != hipSuccess) {
    g_err = "FFT table allocation failed";
    delete c;
    return DCTAE_EHIP;
  }
  c->lds_limit = fft_kernel_setup(device);
  {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0) c->n_cu = cu;
    hipGetLastError();
  }
  hipEventRecord(c->plan_evt, 0);
  *out = c;
  return 0;
}

int dctae_ctx_destroy(dctae_ctx* ctx) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  hipDeviceSynchronize();
  for (auto& kv : ctx->dct) hipFree(kv.second);
  for (auto& kv : ctx->dct_x3) {
    hipFree(kv.second.d);
    hipFree(kv.second.dh);
  }
  for (DevBuf& b : ctx->scratch) b.release();
  ctx->plan.release();
  if (ctx->plan_host) hipHostFree(ctx->plan_host);
  if (ctx->err_dev) hipFree(ctx->err_dev);
  if (ctx->fft_tab) hipFree(ctx->fft_tab);
  drop_encode_plan(ctx);
  for (auto& p : ctx->pending) {
    hipEventDestroy(p.a);
    hipEventDestroy(p.b);
  }
  for (auto e : ctx->evt_pool) hipEventDestroy(e);
  hipEventDestroy(ctx->plan_evt);
  hipEventDestroy(ctx->done_evt);
  if (ctx->side) {
    hipStreamDestroy(ctx->side);
    hipEventDestroy(ctx->side_in);
    hipEventDestroy(ctx->side_out);
  }
  delete ctx;
  return 0;
}

const char* dctae_last_error(dctae_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

// Python passes the reference's exact fp32 colour matrices (util.py:40-41, 91)
int dctae_set_color_matrices(dctae_ctx* ctx, const float* rgb2lms, const float* lms2ipt, const float* ipt2lms,
                             const float* lms2rgb) {
  if (!ctx) return DCTAE_EINVAL;
  std::memcpy(ctx->cm.rgb2lms, rgb2lms, 36);
  std::memcpy(ctx->cm.lms2ipt, lms2ipt, 36);
  std::memcpy(ctx->cm.ipt2lms, ipt2lms, 36);
  std::memcpy(ctx->cm.lms2rgb, lms2rgb, 36);
  return 0;
}

int dctae_set_workspace_limit(dctae_ctx* ctx, int64_t bytes) {
  if (!ctx || bytes < (1 << 20)) return DCTAE_EINVAL;
  ctx->opt.ws_limit = bytes;
  return 0;
}

int dctae_set_fft(dctae_ctx* ctx, int enable) {
  if (!ctx) return DCTAE_EINVAL;
  ctx->opt.fft_enabled = enable != 0;
  return 0;
}

int dctae_set_chunk_bytes(dctae_ctx* ctx, int64_t bytes) {
  if (!ctx || bytes < (1 << 20)) return DCTAE_EINVAL;
  ctx->opt.chunk_bytes = bytes;
  return 0;
}

int dctae_set_option(dctae_ctx* ctx, const char* key, int64_t value) {
  if (!ctx || !key) return DCTAE_EINVAL;
  std::string err;
  const int rc = apply_option(ctx->opt, key, value, &err);
  return rc ? fail(ctx, rc, err) : 0;
}

int dctae_set_timing(dctae_ctx* ctx, int enable) {
  if (!ctx) return DCTAE_EINVAL;
  ctx->timing = enable != 0;
  return 0;
}

int dctae_timing_collect(dctae_ctx* ctx) {
  if (!ctx) return DCTAE_EINVAL;
  for (auto& p : ctx->pending) {
    float ms = 0;
    HIPCHK(ctx, hipEventSynchronize(p.b));
    HIPCHK(ctx, hipEventElapsedTime(&ms, p.a, p.b));
    TimingEntry* e = nullptr;
    for (auto& t : ctx->totals)
      if (t.name == p.name) e = &t;
    if (!e) {
      ctx->totals.push_back({p.name, 0.0, 0});
      e = &ctx->totals.back();
    }
    e->ms += ms;
    e->launches += 1;
    ctx->evt_pool.push_back(p.a);
    ctx->evt_pool.push_back(p.b);
  }
  ctx->pending.clear();
  return 0;
}

int dctae_timing_get(dctae_ctx* ctx, int idx, const char** name, double* total_ms, int64_t* launches) {
  if (!ctx || idx < 0 || idx >= (int)ctx->totals.size()) return DCTAE_EINVAL;
  if (name) *name = ctx->totals[idx].name.c_str();
  if (total_ms) *total_ms = ctx->totals[idx].ms;
  if (launches) *launches = ctx->totals[idx].launches;
  return 0;
}

int dctae_timing_reset(dctae_ctx* ctx) {
  if (!ctx) return DCTAE_EINVAL;
  dctae_timing_collect(ctx);
  ctx->totals.clear();
  return 0;
}

int dctae_check_device_errors(dctae_ctx* ctx, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  int h = 0;
  // a flag raised by the context's previous ordered call on another stream is
  // read only after that call, and a later call's flag is raised after the clear
  OrderedCall oc(ctx, s);
  HIPCHK(ctx, hipMemcpyAsync(&h, ctx->err_dev, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  HIPCHK(ctx, hipMemsetAsync(ctx->err_dev, 0, sizeof(int), s));
  if (h & 1) return fail(ctx, DCTAE_EINVAL, "channel/position index out of range of the PatchNorm tables");
  if (h & 2) return fail(ctx, DCTAE_EINVAL, "batched_image_ids entry has no image (patch_sizes mismatch)");
  if (h & 4) return fail(ctx, DCTAE_EINVAL, "token position outside its image's patch grid");
  if (h & 16) return fail(ctx, DCTAE_EINVAL, "VectorQuantize index out of range of the codebook");
  return 0;
}

int dctae_synth_images(dctae_ctx* ctx, uint64_t seed, int64_t first_index, int32_t n_img, int32_t H, int32_t W,
                       float* rgb_dev, void* stream) {
  if (!ctx || !rgb_dev || n_img < 0 || H < 1 || W < 1) return fail(ctx, DCTAE_EINVAL, "bad synth args");
  if (n_img == 0) return 0;
  Timer t(ctx, (hipStream_t)stream, "synth");
  launch_synth(seed, first_index, n_img, H, W, rgb_dev, (hipStream_t)stream);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_u8_to_f32(dctae_ctx* ctx, const uint8_t* x_dev, int64_t n, float* y_dev, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (n < 0 || (n > 0 && (!x_dev || !y_dev))) return fail(ctx, DCTAE_EINVAL, "bad u8_to_f32 args");
  if (n == 0) return 0;
  hipSetDevice(ctx->device);
  launch_u8_to_f32(x_dev, n, y_dev, (hipStream_t)stream);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dctae_f32_to_u8(dctae_ctx* ctx, const float* x_dev, int64_t n, uint8_t* y_dev, void* stream) {
  if (!ctx) return DCTAE_EINVAL;
  if (n < 0 || (n > 0 && (!x_dev || !y_dev))) return fail(ctx, DCTAE_EINVAL, "bad f32_to_u8 args");
  if (n == 0) return 0;
  hipSetDevice(ctx->device);
  launch_f32_to_u8(x_dev, n, y_dev, (hipStream_t)stream);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

}  // extern "C"
