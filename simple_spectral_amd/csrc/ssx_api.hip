// ssx_api.hip -- C ABI (include/ssx.h) over the gfx950 megakernel.  One translation unit with the
// kernels so the host launches them directly.  No CPU fallback of any kind lives here: every
// entry point either drives the HIP kernels or returns an error.
// The context, its launches, the render worker (render_sample_walk / render_tile_walk behind start_worker), the render entry points and the
// diagnostics are here; scene packing is in ssx_pack.h, RCCL in ssx_rccl.h, the pixel ownership rule in ssx_pixel_grid.h, continue / export /
// import of the sums and the noise estimate (entry points and their kernels) in ssx_progressive.hip, the spectral output in ssx_spectral.hip,
// the guide buffers and the denoising filter in ssx_denoise.hip, the develop of the spectral bins in ssx_develop.hip, their second moments, variances and
// region probes in ssx_spectral_stats.hip, the spectral noise figure in ssx_spectral_noise.hip, the comparison of two spectral renders in ssx_spectral_compare.hip.
#include "ssx_kernels.hip"
#include "ssx_debug.hip"

#include "../../include/ssx.h"

#include <chrono>
#include <array>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <limits.h>
#include <set>

#include "ssx_jit.h"

namespace {

thread_local std::string g_create_error;

// Environment switches of the A/B runs and tests (SSX_GENERIC_KERNEL, SSX_JIT_PASS1, SSX_NARROW_QUEUE, SSX_PRE_HITS).
// None changes a result bit, all change the kernel plan -- so none is looked at unless the master switch SSX_DEBUG_ENV=1 is set:
// a variable inherited from somebody's shell cannot silently change what a production process launches.
const char* debug_env(const char* name) {
	const char* m = getenv("SSX_DEBUG_ENV");
	if (!m || m[0] != '1' || m[1] != '\0') return nullptr;
	return getenv(name);
}
// set and not "0" / empty
bool env_on(const char* name) { const char* e = debug_env(name); return e && e[0] != '\0' && e[0] != '0'; }

std::string fmt(const char* f, ...) {
	char buf[512];
	va_list ap; va_start(ap, f); vsnprintf(buf, sizeof buf, f, ap); va_end(ap);
	return buf;
}

// A device allocation with an owner: freed when the owner goes (with the device current that is current then: ssx_destroy sets the
// context's).  reserve() keeps an allocation that is large enough and otherwise replaces it: the contents are not kept, and it never shrinks.
struct DeviceBuffer {
	void* ptr = nullptr;
	size_t bytes = 0; // capacity
	DeviceBuffer() = default;
	DeviceBuffer(DeviceBuffer&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
	DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { std::swap(ptr, o.ptr); std::swap(bytes, o.bytes); return *this; }
	~DeviceBuffer() { release(); }
	void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
	hipError_t reserve(size_t n) {
		if (n <= bytes) return hipSuccess;
		release();
		const hipError_t e = hipMalloc(&ptr, n);
		if (e == hipSuccess) bytes = n; else ptr = nullptr;
		return e;
	}
	template <class T> T* as() const { return static_cast<T*>(ptr); }
};

} // namespace

#include "ssx_pack.h"

struct ssx_ctx {
	int device = 0;
	int n_cus = 0;                      // compute units of the device (ssx_create)
	hipStream_t stream = nullptr;       // used by the asynchronous start/stop/wait path
	DeviceBuffer d_blob;
	uint32_t blob_words = 0;      // whole blob (generic / calibration / debug kernels stage all of it)
	uint32_t path_blob_words = 0; // what the path kernel stages: without the per-quad vertex table when a specialised kernel runs
	uint32_t topology = 0;        // 0, the built-in mesh topology the scene matched (csrc/ssx_pass1_gen.h), or 3: its own, compiled at upload
	int jit_mode = SSX_JIT_BACKGROUND; // ssx_set_jit: how pass 1 gets specialised for scenes that match no built-in topology
	const ssx_jit::Kernels* jit_kernels[ssx_jit::kVariants] = {}; // [variant: libm, or ssx_jit::kVariantFlux] the run-time compiled kernels of the uploaded scene (topology 3), a mode's when its first render needs them
	uint32_t libm = SSX_LIBM_BUILD; // the libm of the current (or last) render
	uint32_t variant = SSX_LIBM_BUILD; // which kernel twins that render runs (path_kernel_ref): its libm, or ssx_jit::kVariantFlux -- the default libm's _flux twins -- while spectral output is on,
	                                   // or ssx_jit::kVariantPlain -- the default libm's _plain twins -- for a plain render of a plain scene (variant_of)
	// A scene waiting for its own kernels runs the generic one meanwhile: its second blob (packed for topology 3 at upload, the
	// caller's description is gone later) waits on the device, and the context swaps at the start of a render once the code is
	// there (maybe_swap_jit).  The compilation is asked for once the context has launched kJitAfterSamples on the generic kernel.
	bool jit_pending = false, jit_requested = false;
	ssx_jit::VidTable jit_vid;
	DeviceBuffer d_blob_jit; uint32_t blob_jit_words = 0, path_blob_jit_words = 0;
	uint64_t generic_samples = 0;
	int jit_state = SSX_JIT_STATE_NONE; std::string jit_message;
	std::vector<DeviceBuffer> d_textures;
	DeviceBuffer d_jh_data;         // the uplift's table (Jakob-Hanika coefficients / Meng grid)
	bool rgb_mode = false;     // scene uploaded with uplift == SSX_MODE_RGB
	uint32_t scene_traits = 0; // SSX_TRAIT_* of the uploaded scene (scene_traits_of): 0 = its renders may run the kernels with the switches compiled in (variant_of)
	bool fuse_resolve = true;  // false only during the calibration render (no fold: its tail words are read back)
	float calib_frames = 0.0f; // frames per sample measured by the calibration render of ssx_upload_scene
	float calib_left = 0.0f;   // rays per sample that left the scene in it (camera and continuation rays)
	bool pre_hits = false;     // camera rays traced by the generate kernel (SsxKernelArgs::pre_hits): where calib_left pays for it
	DeviceBuffer d_accum;               // the binary64 pixel sums (accum_bytes)
	DeviceBuffer d_unit_counter;        // work-unit counter of the path kernel's persistent waves: four words (enqueue_path)
	int resident_blocks = 0;            // 256-lane path-kernel workgroups the GPU holds at once
	int gen_blocks = 0;                 // the same for the generate kernel
	uint32_t max_wave_slots = 0;        // most waves of the path kernel the GPU can hold: CUs x 16 (ssx_create)
	uint32_t queue_words = SSX_QUEUE_WORDS_WIDE; // entry size of the shadow-ray queues the launches use (pick_queue)
	DeviceBuffer d_samples; // per-sample arrays (ssx_blob.h), one allocation; behind them, in the same allocation, the per-tile and
	                        // per-unit words of a launch (sample_bytes / sample_slots, make_batch)
	DeviceBuffer d_logs;    // the persistent waves' level logs (ssx_blob.h; log_records)
	DeviceBuffer d_out;     // float XYZA image of the asynchronous renders (image_bytes)
	DeviceBuffer d_peer;    // staging buffer of ssx_accumulate_peer (image_bytes)
	bool have_scene = false;
	bool have_cam_dir = false;  // the caller's ssx_scene_desc carried camera.dir

	std::thread worker;
	std::atomic<int> rendering{0};
	std::atomic<int> stop_flag{0};
	std::atomic<uint32_t> done_spp{0};
	std::atomic<uint32_t> done_tiles{0}; // tile_major renders: the device's tiles finished so far (ssx_done_tiles)
	uint32_t total_spp = 0;
	int worker_rc = 0;
	std::atomic<uint64_t> units_enqueued{0}; // work units of every path-kernel launch so far: added to by the worker, read by ssx_units_info
	std::atomic<uint64_t> launches_generated{0}, launches_fused{0}; // launches of a render whose samples ssx_generate_kernel made / the path kernel's refill made (ssx_generate_info)
	ssx_render_params cur{};
	// Progressive rendering (csrc/ssx_progressive.hip).  What d_accum holds -- continuable: every owned pixel holds samples [0, done_spp) of `cur`,
	// the sums may be continued or exported; noise_valid: d_noise describes them, after noise_batches batches (B).  Written by sums_invalidate /
	// sums_publish and, for the estimate, the noise_* helpers; nowhere else.
	// spectral_valid: d_spectral_sums / d_spectral_counts hold the bins of exactly those samples (valid from zero samples or not at all: ssx_spectral.hip).
	// moments_valid: d_spectral_moments holds the second moments of exactly those samples too (the same rule: ssx_spectral_stats.hip).
	// imported: the sums are ssx_sums_import's and nothing has rendered onto them since -- the one state ssx_spectral_import puts the bins next to.
	// spectral_imported: the bins are ssx_spectral_import's, likewise -- the one state ssx_spectral_moments_import puts the moments next to.
	struct SumsState { bool continuable = false, noise_valid = false, spectral_valid = false, moments_valid = false, imported = false, spectral_imported = false; uint32_t noise_batches = 0; } sums;
	uint32_t k_begin = 0;               // first sample of the running call: 0 (ssx_render_start) or the count ssx_render_continue took up (ssx_progress)
	uint64_t scene_digest = 0;          // ssx_scene_digest
	// noise estimate by batch means (ssx_set_noise_estimate): per pixel A_prev | S2 (row-major, 2 x width x height doubles)
	bool noise_on = false;
	DeviceBuffer d_noise;
	DeviceBuffer d_stage;               // row-major staging of ssx_sums_export / ssx_sums_import / ssx_noise_info / ssx_spectral_read: kept from call to call (render_until asks every step)
	// spectral output (ssx_set_spectral_bins; csrc/ssx_spectral.hip): B bins, 0 = off -- then nothing below is allocated, no kernel of it runs and the
	// sample arrays have no flux[].  S[tile slot][bin][pixel of the tile] binary64, N[tile slot][m][pixel of the tile].
	uint32_t spectral_bins = 0;
	DeviceBuffer d_spectral_sums, d_spectral_counts;
	std::string spectral_note;          // why sums that can be continued come without spectral state (ssx_spectral_read says it)
	float lambda_min = 0.0f, lambda_step = 0.0f; // of the uploaded scene
	uint32_t n_quads = 0;      // primitives of the uploaded scene (ssx_debug_step checks its rows against it)
	// spectral moments (ssx_set_spectral_moments; csrc/ssx_spectral_stats.hip): off -- then nothing below is allocated and no kernel of it runs.  Q[tile slot][bin][pixel of
	// the tile] binary64, the layout of S.  d_probe: the row-major arrays, partials and results of ssx_spectral_probe / ssx_probe_arrays and of ssx_spectral_compare / ssx_spectral_compare_arrays; nothing until one of them is called.
	bool spectral_moments = false;
	DeviceBuffer d_spectral_moments, d_probe;
	std::string moments_note;           // why bins that are valid come without moments (ssx_spectral_variance and ssx_spectral_probe say it)
	// denoising (csrc/ssx_denoise.hip): nothing is allocated until ssx_guides / ssx_denoise / ssx_denoise_images is called.  d_guides holds the guide buffers of
	// the uploaded scene at guides_width x guides_height (0: none; ssx_upload_scene drops them), d_denoise the filter's inputs and ping-pong buffers,
	// d_denoise_channels those of the extra channels (ssx_denoise_channels / ssx_denoise_spectral only).
	DeviceBuffer d_guides, d_denoise, d_denoise_channels;
	DeviceBuffer d_develop;             // ssx_develop_images / ssx_spectral_develop (csrc/ssx_develop.hip): weights | output | the caller's bins; nothing until one of them is called
	DeviceBuffer d_optics;              // ssx_optics_images / ssx_spectral_develop_optics (csrc/ssx_optics.hip): two images of bins | the per-bin tables; nothing until one of them is called
	DeviceBuffer d_defocus;             // ssx_defocus_images / ssx_spectral_develop_lens (csrc/ssx_defocus.hip): output | a | inv | focus | distances (| the caller's bins and depth); nothing until a defocus runs
	DeviceBuffer d_sensor;              // ssx_sensor_images / ssx_demosaic_images / ssx_spectral_develop_sensor (csrc/ssx_sensor.hip): the tables | raw | dn | out (| the caller's bins); nothing until one of them is called
	DeviceBuffer d_glare;               // ssx_glare_images / ssx_spectral_develop_glare (csrc/ssx_glare.hip): the chunk's planes X | Kf | the packed twiddles | psf | out (| the caller's bins); nothing until a glare runs
	DeviceBuffer d_display;             // ssx_meter_images / ssx_local_images / ssx_tone_images (csrc/ssx_display.hip): the caller's image | that entry's planes, counters or table; nothing until one of them is called
	uint32_t guides_width = 0, guides_height = 0;
	// demodulated denoising (csrc/ssx_demod.hip): nothing is allocated until ssx_albedo_bins or one of the two _demod entry points is called.  d_albedo_bins
	// holds the albedo bins of the uploaded scene at abins_width x abins_height, abins_bins bins, abins_supersample^2 rays per pixel (0 x 0: none;
	// ssx_upload_scene drops them), d_demod the channel albedo, the demodulated image and variance, the zero albedo guide and the remodulated results.
	DeviceBuffer d_albedo_bins, d_demod;
	uint32_t abins_width = 0, abins_height = 0, abins_bins = 0, abins_supersample = 0;
	uint64_t abins_serial = 0;          // counts the computations of the albedo bins: what the cached channel albedo below was made from
	// the channel albedo r~_c and the zero guide inside d_demod are kept from call to call: made from these albedo bins, weights and floor, in this allocation (nullptr: none)
	const void* demod_rc_base = nullptr; uint64_t demod_rc_bins_serial = 0; float demod_rc_floor = 0.0f; std::vector<float> demod_rc_weights;

	// optional per-kernel timing (ssx_set_timing): events around each stage of each batch
	bool timing = false;
	std::vector<hipEvent_t> ev_pool;   // 6 per batch: gen0, gen1=path0, path1 | three more that close the (empty) resolve and accumulate slots
	size_t ev_used = 0;
	float stage_ms[4] = { 0, 0, 0, 0 };

	// ssx_render_device returns with work still queued on the caller's stream that uses the ctx-owned buffers:
	// later entry points wait for this event before they touch them
	hipEvent_t ev_device_done = nullptr;
	bool device_pending = false;

	// ssx_reduce_rccl: this context's communicator of the group it last combined with (kept for the next combine)
	void* rccl_comm = nullptr; uint64_t rccl_group = 0; int rccl_rank = -1, rccl_size = 0;

	std::mutex error_mutex; // `error` is written by the worker thread and read by ssx_last_error
	std::string error;
	std::string error_out;  // what ssx_last_error hands out (stable until the next call)
};

namespace {

void set_error(ssx_ctx* ctx, const std::string& msg) { std::lock_guard<std::mutex> g(ctx->error_mutex); ctx->error = msg; }

#define SSX_HIP(ctx, call)                                                                          \
	do {                                                                                            \
		hipError_t e_ = (call);                                                                     \
		if (e_ != hipSuccess) {                                                                     \
			set_error((ctx), fmt("%s failed: %s", #call, hipGetErrorString(e_)));                   \
			return SSX_ERR_DEVICE;                                                                  \
		}                                                                                           \
	} while (0)

int fail(ssx_ctx* ctx, int code, const std::string& msg) { set_error(ctx, msg); return code; }

int check_params(ssx_ctx* ctx, const ssx_render_params* p) {
	if (!p || p->struct_size != sizeof(ssx_render_params)) return fail(ctx, SSX_ERR_ARG, "ssx_render_params.struct_size mismatch");
	if (p->libm != SSX_LIBM_BUILD && p->libm != SSX_LIBM_GLIBC_2_35) return fail(ctx, SSX_ERR_ARG, "ssx_render_params.libm: unknown value");
	if (!ctx->have_scene) return fail(ctx, SSX_ERR_STATE, "no scene uploaded");
	if (p->width == 0 || p->height == 0 || p->spp == 0) return fail(ctx, SSX_ERR_ARG, "width, height and spp must be positive");
	if ((uint64_t)p->width * p->height > (1ull << 28)) return fail(ctx, SSX_ERR_ARG, "image too large");
	if (p->tile_stride == 0 || p->tile_first >= p->tile_stride) return fail(ctx, SSX_ERR_ARG, "need tile_first < tile_stride");
	if (p->no_flat_field_correction && !ctx->have_cam_dir) return fail(ctx, SSX_ERR_ARG, "no_flat_field_correction needs ssx_scene_desc.cam_dir (caller built against an older ssx.h)");
	return SSX_OK;
}

// The caller's parameters as this library's struct: a caller built before ssx_render_params.libm (struct_size = offsetof(.., libm)) gets
// SSX_LIBM_BUILD.  Then check_params.
int take_params(ssx_ctx* ctx, const ssx_render_params* in, ssx_render_params* out) {
	if (!in) return fail(ctx, SSX_ERR_ARG, "ssx_render_params is NULL");
	memset(out, 0, sizeof *out);
	if (in->struct_size == offsetof(ssx_render_params, libm)) { memcpy(out, in, offsetof(ssx_render_params, libm)); out->struct_size = sizeof *out; }
	else memcpy(out, in, in->struct_size == sizeof *out ? sizeof *out : sizeof out->struct_size);
	return check_params(ctx, out);
}
// ... and no asynchronous render running (`busy`: what the entry point calls that)
int begin_render(ssx_ctx* ctx, const ssx_render_params* in, ssx_render_params* out, const char* busy) {
	const int rc = take_params(ctx, in, out);
	if (rc) return rc;
	return ctx->rendering.load() ? fail(ctx, SSX_ERR_STATE, busy) : SSX_OK;
}

// a render queued by ssx_render_device uses the context's buffers: whoever is about to touch them from the host waits for it
int wait_device_pending(ssx_ctx* ctx) {
	if (ctx->device_pending) { SSX_HIP(ctx, hipEventSynchronize(ctx->ev_device_done)); ctx->device_pending = false; }
	return SSX_OK;
}

// What the entry points that neither start a render nor need the context's sums ask first: no render running; then the context's device is current and
// nothing queued by ssx_render_device is left on it.
int idle_on_device(ssx_ctx* ctx) {
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	return wait_device_pending(ctx);
}

uint32_t tiles_across(uint32_t pixels) { return (pixels + 7u) / 8u; } // 8x8 tiles along a width or a height
// The pixel sums are laid out per 8x8 tile as [tile][X, Y, Z, alpha][pixel of the tile] (binary64), so that the 64 lanes of a
// folding wave read and write 512 consecutive bytes per component: one slot per pixel of every (whole) tile of the image.
size_t accum_bytes(uint32_t width, uint32_t height) { return (size_t)tiles_across(width) * tiles_across(height) * 64u * 4 * sizeof(double); }
size_t image_bytes(uint32_t width, uint32_t height) { return (size_t)width * height * 4 * sizeof(float); } // float XYZA (d_out, d_peer)

SsxPixelGrid pixel_grid(const ssx_render_params* p) { // (tile_skew reduced as in make_plan)
	const uint32_t tx = tiles_across(p->width);
	return SsxPixelGrid{ p->width, p->height, tx, p->tile_first, p->tile_stride, p->tile_skew % tx };
}
// how many of the image's 8x8 tiles the context owns: tiles tile_first, tile_first + tile_stride, ... of the (skewed) tile list
uint32_t owned_tiles(const ssx_render_params& p) {
	const uint32_t n_tiles = tiles_across(p.width) * tiles_across(p.height);
	return n_tiles > p.tile_first ? (n_tiles - p.tile_first + p.tile_stride - 1u) / p.tile_stride : 0u;
}
dim3 pixel_blocks(const ssx_render_params* p) { return dim3((p->width * p->height + 255u) / 256u); } // the grid of a per-pixel kernel

int clear_sums(ssx_ctx* ctx, uint32_t width, uint32_t height, hipStream_t stream) {
	SSX_HIP(ctx, hipMemsetAsync(ctx->d_accum.ptr, 0, accum_bytes(width, height), stream));
	return SSX_OK;
}
// Whoever is about to overwrite or reinterpret d_accum (another render, another scene, an import) says so first; a render that fails leaves it at that.
void sums_invalidate(ssx_ctx* ctx) { ctx->sums = ssx_ctx::SumsState{}; }
// ... and whoever leaves samples [0, done_spp) of ctx->cur in every owned pixel says that.  (noise_batches: the estimate arrived with the sums, ssx_sums_import.)
void sums_publish(ssx_ctx* ctx, uint32_t done_spp, int64_t noise_batches = -1) {
	if (noise_batches >= 0) { ctx->sums.noise_valid = true; ctx->sums.noise_batches = (uint32_t)noise_batches; }
	ctx->done_spp.store(done_spp); ctx->sums.continuable = true;
}

// Every launch keeps 48 bytes per sample ([tile slot][k][64]: camera ray, stream / tail word, camera hit) from the generate
// kernel until the path kernel has folded the sample; the buffer bounds how many samples per pixel one launch may cover.  The
// levels of the recursion live in the persistent waves' logs (ensure_logs), whose size does not depend on the launch.
constexpr size_t kSampleBufferBudget = (size_t)16 << 30; // bytes of per-sample arrays one launch may use (512^2 x 256 spp = 3.2 GB; 16 GiB = 358 M samples ~ 110 ms of rendering)
// (64 while spectral output is on: the fold of the _flux kernels leaves every sample's hero flux in a fourth array, ssx_blob.h)
size_t bytes_per_sample(const ssx_ctx* ctx) { return ctx->spectral_bins ? SSX_BYTES_PER_SAMPLE_FLUX : SSX_BYTES_PER_SAMPLE; }
// Behind the per-sample arrays, per launch: unit_state (1 word per work unit) and tile_mask (4 words per tile slot).  A launch of R records
// has at most R / 64 tile slots and R / 64 units: 5 words per 64 records bound both, so the words are part of the sample allocation
// (sized before anything is enqueued: ensure_samples) and never grown in the enqueue path.
constexpr size_t kAuxWordsPer64Records = 5;
size_t bytes_per_64_records(const ssx_ctx* ctx) { return 64u * bytes_per_sample(ctx) + kAuxWordsPer64Records * sizeof(uint32_t); }
size_t sample_bytes(const ssx_ctx* ctx, size_t records) { return records / 64u * bytes_per_64_records(ctx); } // the allocation for `records` (64 per tile and sample: a multiple of 64)
size_t sample_slots(const ssx_ctx* ctx) { return ctx->d_samples.bytes / bytes_per_64_records(ctx) * 64u; } // record capacity of the allocation
size_t log_records(const ssx_ctx* ctx) { return ctx->d_logs.bytes / SSX_LOG_BYTES_PER_RECORD; }     // log-record capacity
constexpr uint32_t kMinUnits = 3072;                   // one wave work unit per wave slot of the GPU (256 CUs x 4 SIMDs x 3 waves)
// Samples an asynchronous render launches between two host synchronisations, about (~20 ms): the granularity of progress and ssx_render_stop, large
// enough that the synchronisation between launches stays a few percent.
constexpr uint64_t kSamplesPerSync = (uint64_t)32 << 20;

struct LaunchPlan { SsxKernelArgs args; uint32_t max_spp_per_launch; };

// The render switches the reference fixes at compile time (stdafx.hpp) and this library takes at run time.  A scene and a render
// with none of these traits are "plain": the path kernels exist a second time with exactly that compiled in (render_body's PLAIN, the _plain
// twins), without the tests on the switches in their loop.
// Scene side, from the description (what pack_blob writes into the quad records and the header): a quad on a mirror material, a top-level
// triangle among the lights, an uplift other than "ours".  (Malformed indices are pack_blob's to refuse: skipped here.)
uint32_t scene_traits_of(const ssx_scene_desc* s) {
	uint32_t t = 0;
	for (uint32_t q = 0; q < s->n_quads; ++q) if (s->quads[q].material < s->n_materials && s->materials[s->quads[q].material].kind != SSX_MTL_LAMBERTIAN) t |= SSX_TRAIT_MIRROR;
	for (uint32_t i = 0; i < s->n_lights; ++i) if (s->lights[i] < s->n_quads && (s->quads[s->lights[i]].flags & SSX_PRIM_TRI)) t |= SSX_TRAIT_TRI_LIGHT;
	if (s->uplift == SSX_MODE_RGB) t |= SSX_TRAIT_RGB_MODE;
	else if (s->uplift != SSX_UPLIFT_OURS) t |= SSX_TRAIT_UPLIFT;
	return t;
}
// Render side, from the parameters (take_params' struct); keep_samples is the entry point's (ssx_debug_samples).
uint32_t render_traits_of(const ssx_render_params* p, bool keep_samples) {
	return (p->indirect_only ? SSX_TRAIT_INDIRECT_ONLY : 0u) | (p->no_explicit_light_sampling ? SSX_TRAIT_NO_ELS : 0u) |
	       (p->no_flat_field_correction ? SSX_TRAIT_NO_FLAT_FIELD : 0u) | (keep_samples ? SSX_TRAIT_KEEP_SAMPLES : 0u) | (p->libm != SSX_LIBM_BUILD ? SSX_TRAIT_LIBM : 0u);
}
// Everything that keeps a render of the context off the _plain kernels: the two above, spectral output (its _flux twins keep the general body) and
// SSX_PLAIN_KERNEL=0 (under SSX_DEBUG_ENV=1: A/B runs and tests).
uint32_t traits_of(const ssx_ctx* ctx, const ssx_render_params* p, bool keep_samples) {
	const char* e = debug_env("SSX_PLAIN_KERNEL");
	return ctx->scene_traits | render_traits_of(p, keep_samples) | (ctx->spectral_bins ? SSX_TRAIT_SPECTRAL_BINS : 0u) | (e && e[0] == '0' ? SSX_TRAIT_FORCED_OFF : 0u);
}
// Which kernel twins a render runs (ssx_ctx::variant).  Decided for EVERY render from its own parameters and the context's state at that moment
// (ready_to_launch): nothing of an earlier render's choice is kept.
uint32_t variant_of(const ssx_ctx* ctx, const ssx_render_params* p, bool keep_samples = false) {
	if (ctx->spectral_bins && p->libm == SSX_LIBM_BUILD && !ctx->rgb_mode) return ssx_jit::kVariantFlux;
	return traits_of(ctx, p, keep_samples) == 0u ? (uint32_t)ssx_jit::kVariantPlain : p->libm;
}

LaunchPlan make_plan(ssx_ctx* ctx, const ssx_render_params* p, bool ask_device = true) {
	LaunchPlan pl{};
	SsxKernelArgs& a = pl.args;
	a.blob = ctx->d_blob.as<uint32_t>(); a.blob_words = ctx->path_blob_words;
	a.width = p->width; a.height = p->height;
	a.inv_width = 1.0 / (double)p->width; a.inv_height = 1.0 / (double)p->height;
	a.tiles_x = tiles_across(p->width);
	a.n_tiles = a.tiles_x * tiles_across(p->height);
	// tile_skew only ever enters as (ty * tile_skew) % tiles_x: reduced here, so that the kernels' 32-bit product cannot wrap where the
	// hosts' wider arithmetic (host/renderer.cpp, simple_spectral_amd/dist.py) does not -- any skew names the same tile list everywhere
	a.tile_first = p->tile_first; a.tile_stride = p->tile_stride; a.tile_skew = p->tile_skew % a.tiles_x;
	a.indirect_only = p->indirect_only ? 1u : 0u;
	a.no_els = p->no_explicit_light_sampling ? 1u : 0u;
	a.no_flat_field = p->no_flat_field_correction ? 1u : 0u;
	a.seed = p->seed;
	a.rgb_mode = ctx->rgb_mode ? 1u : 0u;
	a.fuse_resolve = ctx->fuse_resolve ? 1u : 0u;
	a.pre_hits = ctx->pre_hits ? 1u : 0u;
	a.my_tiles = owned_tiles(*p);
	size_t per_spp = (size_t)(a.my_tiles ? a.my_tiles : 1u) * 64u * bytes_per_sample(ctx);
	// the budget, or 80 % of what is free on the device right now (plus what this context already holds)
	size_t budget = kSampleBufferBudget, free_b = 0, total_b = 0;
	if (ask_device && hipMemGetInfo(&free_b, &total_b) == hipSuccess) { // (not while the stream is being captured: the buffers have their size then)
		const size_t avail = (size_t)((double)(free_b + sample_slots(ctx) * bytes_per_sample(ctx)) * 0.8);
		if (avail < budget) budget = avail;
	}
	size_t cap = budget / per_spp;
	// record indices are 32-bit in the kernels
	const size_t idx_cap = (size_t)0xFFFFFFFFu / ((size_t)(a.my_tiles ? a.my_tiles : 1u) * 64u);
	if (cap > idx_cap) cap = idx_cap;
	pl.max_spp_per_launch = (uint32_t)(cap < 1 ? 1 : (cap > 65536 ? 65536 : cap));
	return pl;
}

// A render recorded into a hipGraph (ssx_render_device while the stream is capturing) cannot ask the device for its free memory and
// cannot grow a buffer: the samples per pixel one of its launches may cover follow from the sample arrays the context already holds --
// a budget in RECORDS, so it holds whatever the captured render's image size and tile split are (the cap used to be the
// earlier render's, in ITS samples per pixel).  Nothing fits: the cap stays, and the caller reports that the buffers would have to grow.
void cap_to_allocation(const ssx_ctx* ctx, LaunchPlan& pl) {
	const size_t per_spp = (size_t)(pl.args.my_tiles ? pl.args.my_tiles : 1u) * 64u;
	const size_t fit = sample_slots(ctx) / per_spp;
	if (fit >= 1 && fit < pl.max_spp_per_launch) pl.max_spp_per_launch = (uint32_t)fit;
}

int ensure_samples(ssx_ctx* ctx, const LaunchPlan& pl, uint32_t n_k) {
	const size_t need = (size_t)pl.args.my_tiles * 64u * n_k;
	const hipError_t e = ctx->d_samples.reserve(sample_bytes(ctx, need));
	if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(ctx, SSX_ERR_DEVICE, fmt("out of device memory for %zu samples in flight; lower spp_per_launch", need)); }
	SSX_HIP(ctx, e);
	return SSX_OK;
}

// The persistent waves' level logs: one region per wave slot, unit tag and cohort (ssx_blob.h).  A CU holds at most 16
// waves of the path kernel (4 per SIMD at 128 VGPRs), whichever variant runs.
int ensure_logs(ssx_ctx* ctx, uint32_t unit_cohorts) {
	const size_t need = (size_t)ctx->max_wave_slots * 2u * unit_cohorts * SSX_COHORT_RECORDS, bytes = need * SSX_LOG_BYTES_PER_RECORD;
	if (bytes >= ((size_t)1 << 32)) return fail(ctx, SSX_ERR_DEVICE, "level logs beyond 4 GiB: the kernels address them with 32-bit offsets");
	if (ctx->d_logs.bytes >= bytes) return SSX_OK;
	// Sized once per scene for the largest unit it renders with (calibrate), so this does not happen on the enqueue path of a
	// render; should it (a debugging variable enlarging the units), the old logs may still serve a queued render of this
	// context: wait for THAT -- the event of ssx_render_device and the context's own stream -- not for the whole device.
	if (ctx->d_logs.ptr) {
		const int rc = wait_device_pending(ctx);
		if (rc) return rc;
		SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	}
	const hipError_t e = ctx->d_logs.reserve(bytes);
	if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(ctx, SSX_ERR_DEVICE, fmt("out of device memory for the level logs (%zu bytes)", bytes)); }
	SSX_HIP(ctx, e);
	return SSX_OK;
}

// the per-sample arrays of one batch inside a region of `cap` records starting at `base`, and the waves' logs (ssx_blob.h)
void bind_arrays(SsxKernelArgs& a, uint8_t* base, uint64_t cap, uint8_t* logs, uint64_t log_cap, bool with_flux) {
	a.ray = reinterpret_cast<float4*>(base);                      base += cap * 16u;
	a.st = reinterpret_cast<uint4*>(base);                        base += cap * 16u;
	a.hit = reinterpret_cast<float4*>(base);                      base += cap * 16u;
	a.flux = with_flux ? reinterpret_cast<float4*>(base) : nullptr; // (spectral output on: the allocation counts 64 bytes per record)
	a.logs = logs; a.log_cap = (uint32_t)log_cap; // fs | nee | direct | np | link | vis (ssx_kernels.hip: log_fs ...)
}

// adds the stage durations of the recorded batches to ctx->stage_ms
int collect_timing(ssx_ctx* ctx) {
	for (size_t b = 0; b + 6 <= ctx->ev_used; b += 6) {
		hipEvent_t* e = &ctx->ev_pool[b];
		SSX_HIP(ctx, hipEventSynchronize(e[2]));
		SSX_HIP(ctx, hipEventSynchronize(e[5]));
		const int pairs[4][2] = { { 0, 1 }, { 1, 2 }, { 3, 4 }, { 4, 5 } };
		for (int k = 0; k < 4; ++k) {
			float ms = 0;
			SSX_HIP(ctx, hipEventElapsedTime(&ms, e[pairs[k][0]], e[pairs[k][1]]));
			ctx->stage_ms[k] += ms;
		}
	}
	ctx->ev_used = 0;
	return SSX_OK;
}

int timing_events(ssx_ctx* ctx, hipEvent_t** out) {
	if (ctx->ev_used + 6 > 6 * 64) { int r = collect_timing(ctx); if (r) return r; }
	while (ctx->ev_pool.size() < ctx->ev_used + 6) {
		hipEvent_t e;
		// timing only: without the system-scope fence (cache write-back + invalidation) a default event puts between two kernels
		SSX_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
		ctx->ev_pool.push_back(e);
	}
	*out = &ctx->ev_pool[ctx->ev_used];
	ctx->ev_used += 6;
	return SSX_OK;
}

// One batch = samples [k0,k1) of every owned pixel: generate (camera rays, and their hits where the scene pre-traces them) ->
// path megakernel (every further level, the fold of the recursion, flux -> XYZ and the ordered binary64 pixel sums).
struct Batch { SsxKernelArgs a; uint32_t units; uint64_t n_rec; hipEvent_t* tev; int rc; };

// samples per pixel of a work unit for the uploaded scene (before make_batch halves it for small launches)
uint32_t unit_spp_of(const ssx_ctx* ctx) { return ctx->calib_frames >= 2.0f ? SSX_MAX_UNIT_KS / 2u : SSX_MAX_UNIT_KS; }

Batch make_batch(ssx_ctx* ctx, const LaunchPlan& pl, uint32_t k0, uint32_t k1) {
	Batch b{};
	b.a = pl.args;
	SsxKernelArgs& a = b.a;
	const uint32_t n_k = k1 - k0;
	a.k0 = k0; a.k1 = k1;
	a.n_records = (uint64_t)a.my_tiles * n_k * 64u;
	// Samples per pixel and unit.  Long paths (Cornell: 4 continued levels per sample) run best with 4 -- 256 items keep the
	// refill busy, less of a unit's logs is in flight per wave, and short units balance the end of the launch: 3052 against
	// 3016 Msamples/s with 8, 3031 with 2, 2899 with 16 (one box) --, short ones (plane-srgb: 1 level) with 8: 10.07 against
	// 9.89 Gsamples/s.  Halved while the launch is so small that SIMDs would be left without a wave (3 waves x 1024 SIMDs).
	uint32_t g = unit_spp_of(ctx);
	while (g > 1u && (uint64_t)((n_k + g - 1u) / g) * a.my_tiles < kMinUnits) g >>= 1;
	a.group_spp = g;
	if (a.group_spp > n_k) a.group_spp = n_k;
	a.unit_cohorts = (a.group_spp + SSX_COHORT_KS - 1u) / SSX_COHORT_KS;
	// units per grab (ssx_kernels.hip rotate_fetch): four where paths are short and a wave's lanes run dry together (plane-srgb: +0.9 %), one where they are
	// long (Cornell box: four cost 0.3 %)
	a.unit_grab = ctx->calib_frames >= 2.0f ? 1u : 4u;
	// (ssx_kernels.hip rotate_fetch keeps what is left of a grab in five bits, and units without samples or cohorts are none: the device checks neither)
	if (a.unit_grab < 1u || a.unit_grab > 32u || a.group_spp == 0u || a.unit_cohorts == 0u) {
		b.rc = fail(ctx, SSX_ERR_STATE, fmt("internal: launch with unit_grab = %u (1..32), group_spp = %u, unit_cohorts = %u", a.unit_grab, a.group_spp, a.unit_cohorts));
		return b;
	}
	a.n_groups = (n_k + a.group_spp - 1) / a.group_spp;
	b.units = a.my_tiles * a.n_groups;
	b.n_rec = a.n_records;
	// sample arrays and logs are shared by all batches of a render: their kernels run one after the other in stream order
	b.rc = ensure_logs(ctx, a.unit_cohorts);
	if (b.rc == SSX_OK) bind_arrays(a, ctx->d_samples.as<uint8_t>(), a.n_records, ctx->d_logs.as<uint8_t>(), log_records(ctx), ctx->spectral_bins != 0u);
	a.accum = ctx->d_accum.as<double>();
	// the launch's per-unit and per-tile words, behind the sample arrays' capacity: unit_state | tile_mask
	uint32_t* const aux = reinterpret_cast<uint32_t*>(ctx->d_samples.as<uint8_t>() + sample_slots(ctx) * bytes_per_sample(ctx));
	a.unit_state = aux;
	a.tile_mask = aux + b.units;
	if (b.rc == SSX_OK && (size_t)a.my_tiles * 4u + b.units > (sample_slots(ctx) / 64u) * kAuxWordsPer64Records) b.rc = fail(ctx, SSX_ERR_STATE, "internal: launch larger than the sample allocation");
	return b;
}

// dynamic LDS of a kernel that stages `blob_words` of the blob (ssx_kernels.hip stage_lds): the coefficient table in front of them
size_t staged_blob_lds(uint32_t blob_words) { return ((size_t)blob_words + SSX_LDS_PREFIX_WORDS) * 4; }
// ... and of a path-kernel workgroup: that + 4 waves' shadow-ray queues and log counters
size_t path_lds_bytes(uint32_t blob_words, uint32_t queue_words) {
	size_t n = staged_blob_lds(blob_words) + 4u * ((size_t)SSX_QUEUE_ENTRIES * queue_words + SSX_WAVE_COUNTER_WORDS) * 4u;
#ifdef SSX_REGTIME // profiling build: the waves' region timers (ssx_lanestat.h SSX_TIME)
	n += 4u * SSX_NTIME * 8u;
#endif
	return n;
}
// The path megakernels of this library: [variant: libm 0 / 1, 2 = the default libm's _flux twins (spectral output), or 3 = its _plain twins (the render switches compiled in: variant_of)][pass-1 variant: 0 generic, 1 Cornell
// topology, 2 plane topology][narrow queue entries].
// Topology 3 runs the run-time compiled pair of the scene's pattern (ssx_ctx::jit_kernels), named the same in both modes (other modules).
struct PathKernel { const char* name; void (*host)(SsxKernelArgs); };
#define SSX_PK(k) { #k, k }
static const PathKernel kPathKernels[ssx_jit::kVariants][3][2] = {
	{ { SSX_PK(ssx_render_kernel), SSX_PK(ssx_render_kernel_nq) }, { SSX_PK(ssx_render_kernel_cornell), SSX_PK(ssx_render_kernel_cornell_nq) },
	  { SSX_PK(ssx_render_kernel_plane), SSX_PK(ssx_render_kernel_plane_nq) } },
	{ { SSX_PK(ssx_render_kernel_glibc), SSX_PK(ssx_render_kernel_nq_glibc) }, { SSX_PK(ssx_render_kernel_cornell_glibc), SSX_PK(ssx_render_kernel_cornell_nq_glibc) },
	  { SSX_PK(ssx_render_kernel_plane_glibc), SSX_PK(ssx_render_kernel_plane_nq_glibc) } },
	{ { SSX_PK(ssx_render_kernel_flux), SSX_PK(ssx_render_kernel_nq_flux) }, { SSX_PK(ssx_render_kernel_cornell_flux), SSX_PK(ssx_render_kernel_cornell_nq_flux) },
	  { SSX_PK(ssx_render_kernel_plane_flux), SSX_PK(ssx_render_kernel_plane_nq_flux) } },
	{ { SSX_PK(ssx_render_kernel_plain), SSX_PK(ssx_render_kernel_nq_plain) }, { SSX_PK(ssx_render_kernel_cornell_plain), SSX_PK(ssx_render_kernel_cornell_nq_plain) },
	  { SSX_PK(ssx_render_kernel_plane_plain), SSX_PK(ssx_render_kernel_plane_nq_plain) } } };
#undef SSX_PK
static const char* const kJitKernelNames[2] = { "ssx_render_kernel_jit", "ssx_render_kernel_jit_nq" };
// this library's kernel for the context's libm and topology (a scene still waiting for its own kernels runs the generic one)
const PathKernel& path_kernel_of(const ssx_ctx* ctx, bool narrow) { return kPathKernels[ctx->variant][ctx->topology < 3u ? ctx->topology : 0u][narrow]; }
// A kernel of this library (host function) or of a run-time compiled module (topology 3), for the context's libm.  A glibc-mode render of a
// specialised scene has its kernels (ensure_libm_kernels) before it gets here.
struct KernelRef { const void* host = nullptr; hipFunction_t mod = nullptr; };
KernelRef path_kernel_ref(const ssx_ctx* ctx, bool narrow) {
	KernelRef k;
	const ssx_jit::Kernels* jk = ctx->jit_kernels[ctx->variant];
	if (ctx->topology == 3u && jk) k.mod = narrow ? jk->path_nq : jk->path;
	else k.host = (const void*)path_kernel_of(ctx, narrow).host;
	return k;
}
int occupancy_of(ssx_ctx* ctx, const KernelRef& k, size_t lds, int* per_cu) {
	if (k.mod) SSX_HIP(ctx, hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, k.mod, 256, lds));
	else SSX_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, k.host, 256, lds));
	return SSX_OK;
}
// 256-lane workgroups of kernel `k` with `lds` bytes of dynamic LDS that the GPU holds at once (one per CU where the query finds room for none)
int blocks_that_fit(ssx_ctx* ctx, const KernelRef& k, size_t lds, int* blocks) {
	int per_cu = 0;
	const int rc = occupancy_of(ctx, k, lds, &per_cu);
	if (rc) return rc;
	*blocks = (per_cu > 0 ? per_cu : 1) * ctx->n_cus;
	return SSX_OK;
}
int launch_kernel(ssx_ctx* ctx, const KernelRef& k, uint32_t blocks, size_t lds, hipStream_t stream, SsxKernelArgs& a) {
	if (k.mod) {
		size_t size = sizeof a;
		void* config[] = { HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END };
		SSX_HIP(ctx, hipModuleLaunchKernel(k.mod, blocks, 1, 1, 256, 1, 1, (unsigned)lds, stream, nullptr, config));
	} else {
		void* args[] = { &a };
		SSX_HIP(ctx, hipLaunchKernel(k.host, dim3(blocks), dim3(256), args, lds, stream));
	}
	return SSX_OK;
}
// Wide queue entries (ssx_blob.h) unless the narrow ones let one more workgroup live on a CU (or only they fit at all).
int pick_queue(ssx_ctx* ctx, uint32_t blob_words, uint32_t* queue_words, int* blocks_per_cu) {
	int wide = 0, narrow = 0, rc;
	if (path_lds_bytes(blob_words, SSX_QUEUE_WORDS_WIDE) <= 65536u)
		if ((rc = occupancy_of(ctx, path_kernel_ref(ctx, false), path_lds_bytes(blob_words, SSX_QUEUE_WORDS_WIDE), &wide))) return rc;
	if ((rc = occupancy_of(ctx, path_kernel_ref(ctx, true), path_lds_bytes(blob_words, SSX_QUEUE_WORDS_NARROW), &narrow))) return rc;
	const bool use_narrow = narrow > wide || env_on("SSX_NARROW_QUEUE"); // the variable: tests and A/B runs
	*queue_words = use_narrow ? SSX_QUEUE_WORDS_NARROW : SSX_QUEUE_WORDS_WIDE;
	if (blocks_per_cu) *blocks_per_cu = use_narrow ? narrow : wide;
	return SSX_OK;
}

// Kernels of the plane topology make their samples in the path loop where camera rays are traced there anyway (SsxKernelArgs::fuse_gen,
// ssx_kernels.hip refill): no generate kernel for such a launch of a render.  (SSX_FUSE_GEN=0 under SSX_DEBUG_ENV=1: A/B runs and tests.)
bool fuses_generate(const ssx_ctx* ctx, const SsxKernelArgs& a) {
	const char* fuse_env = debug_env("SSX_FUSE_GEN");
	// (the unit carries its tile's column and row in 16 bits each: WorkUnit::txy -- an image more than 524 280 pixels wide or high keeps the generate kernel)
	const bool tiles_fit = a.tiles_x <= 0xFFFFu && tiles_across(a.height) <= 0xFFFFu;
	return ctx->topology == 2u && !a.pre_hits && tiles_fit && !(fuse_env && fuse_env[0] == '0');
}

// Camera rays + (where the scene pre-traces them) their closest hits: persistent workgroups striding over the record waves; they stage
// the whole blob -- the trace is the generic one, restricted per tile to the primitives its frustum can contain (ssx_tile_mask_kernel,
// a few microseconds).  (The per-tile and per-unit words of the launch live behind the sample arrays: make_batch.)
int enqueue_generate(ssx_ctx* ctx, const Batch& b, hipStream_t stream) {
	SsxKernelArgs ga = b.a;
	ga.blob_words = ctx->blob_words;
	if (ga.pre_hits) {
		hipLaunchKernelGGL(ssx_tile_mask_kernel, dim3((ga.my_tiles + 3u) / 4u), dim3(256), 0, stream, ga);
		SSX_HIP(ctx, hipGetLastError());
	}
	const KernelRef gen_kernel{ (const void*)ssx_generate_kernel };
	const size_t gen_lds = staged_blob_lds(ga.blob_words);
	if (ctx->gen_blocks == 0) { const int rc = blocks_that_fit(ctx, gen_kernel, gen_lds, &ctx->gen_blocks); if (rc) return rc; }
	const uint64_t want = (b.n_rec + 255u) / 256u;
	return launch_kernel(ctx, gen_kernel, (uint32_t)(want < (uint64_t)ctx->gen_blocks ? want : (uint64_t)ctx->gen_blocks), gen_lds, stream, ga);
}

// A path kernel over the batch's work units.  Persistent waves: as many workgroups as the GPU holds at once (`resident_blocks`; or
// fewer, for a small launch); they fetch work units from a counter.  The kernel stages `blob_words` of the blob.
int enqueue_path(ssx_ctx* ctx, Batch& b, const KernelRef& kernel, uint32_t queue_words, uint32_t blob_words, int resident_blocks, hipStream_t stream) {
	if (!ctx->d_unit_counter.ptr) { // [1]: rays that left the scene (calibration render); [2], [3]: units parked / added by the wave in front (ssx_sums_info; never reset)
		SSX_HIP(ctx, ctx->d_unit_counter.reserve(4 * sizeof(uint32_t)));
		SSX_HIP(ctx, hipMemsetAsync(ctx->d_unit_counter.ptr, 0, 4 * sizeof(uint32_t), stream));
	}
	b.a.blob_words = blob_words; b.a.queue_words = queue_words;
	SSX_HIP(ctx, hipMemsetAsync(ctx->d_unit_counter.ptr, 0, 2 * sizeof(uint32_t), stream));
	SSX_HIP(ctx, hipMemsetAsync(b.a.unit_state, 0, (size_t)b.units * sizeof(uint32_t), stream));
	b.a.unit_counter = ctx->d_unit_counter.as<uint32_t>();
	const uint32_t want_blocks = (b.units + 3u) / 4u;
	uint32_t blocks = want_blocks < (uint32_t)resident_blocks ? want_blocks : (uint32_t)resident_blocks;
	if (blocks * 4u > ctx->max_wave_slots) blocks = ctx->max_wave_slots / 4u; // every wave of the grid owns a log region
	return launch_kernel(ctx, kernel, blocks, path_lds_bytes(blob_words, queue_words), stream, b.a);
}

// One batch of a render, in stream order: (timing event) -> [tile mask ->] [generate ->] (event) -> path kernel of the context's libm
// and topology, with the queue entries pick_queue chooses -> (four events).
int launch_batch(ssx_ctx* ctx, Batch& b, hipStream_t stream) {
	if (b.rc) return b.rc; // make_batch refused the launch, or could not get the waves' logs
	int rc;
	// (a _plain kernel does not look at the switches: a launch that carries one must never reach it)
	if (ctx->variant == ssx_jit::kVariantPlain && (b.a.indirect_only | b.a.no_els | b.a.no_flat_field | b.a.rgb_mode | b.a.keep_samples | ctx->scene_traits))
		return fail(ctx, SSX_ERR_STATE, "internal: a render with a switch set was about to launch the kernel with the switches compiled in");
	if (ctx->timing) { if ((rc = timing_events(ctx, &b.tev))) return rc; SSX_HIP(ctx, hipEventRecord(b.tev[0], stream)); }
	b.a.fuse_gen = fuses_generate(ctx, b.a) ? 1u : 0u;
	if (!b.a.fuse_gen && (rc = enqueue_generate(ctx, b, stream))) return rc;
	if (ctx->timing) SSX_HIP(ctx, hipEventRecord(b.tev[1], stream));
	// (the plan -- queue entries, resident workgroups -- is kept until an upload, another libm or the scene's own kernels change the kernel or its LDS)
	const bool plan = ctx->resident_blocks == 0;
	if (plan && (rc = pick_queue(ctx, b.a.blob_words, &ctx->queue_words, nullptr))) return rc;
	const KernelRef path_kernel = path_kernel_ref(ctx, ctx->queue_words == SSX_QUEUE_WORDS_NARROW);
	if (plan && (rc = blocks_that_fit(ctx, path_kernel, path_lds_bytes(b.a.blob_words, ctx->queue_words), &ctx->resident_blocks))) return rc;
	if ((rc = enqueue_path(ctx, b, path_kernel, ctx->queue_words, b.a.blob_words, ctx->resident_blocks, stream))) return rc;
	ctx->units_enqueued.fetch_add(b.units);
	(b.a.fuse_gen ? ctx->launches_fused : ctx->launches_generated).fetch_add(1u);
	if (ctx->timing) for (int k = 2; k < 6; ++k) SSX_HIP(ctx, hipEventRecord(b.tev[k], stream)); // (fold and pixel sums ran inside the path kernel: their slots stay ~0)
	return SSX_OK;
}

// A scene that waits for kernels of its own (ssx_upload_scene): are they there?  Called at the start of a render (and between the
// launches of an asynchronous one), `samples` = what the caller is about to launch.  Ready: the context switches to its second
// blob and the compiled kernels -- work already queued keeps the first blob, which stays allocated -- ; not asked for yet: the
// compilation is requested once the generic kernel has served kJitAfterSamples (a test's 8 x 8 image is not worth a core-second
// of hipRTC; a production render passes the mark in its first launch and has its kernels a second or two later).
constexpr uint64_t kJitAfterSamples = kSamplesPerSync; // (a threshold of its own meaning, tied to the launch size by "in its first launch")
// The kernels asked for and looked for are those of the render's libm (ctx->libm): each mode's first code object of the pattern comes the
// same way; the other mode's, should a render of it follow the swap, is compiled by ensure_libm_kernels.
void maybe_swap_jit(ssx_ctx* ctx, uint64_t samples) {
	if (!ctx->jit_pending) return;
	std::string err;
	const ssx_jit::Kernels* k = nullptr;
	const ssx_jit::State st = ssx_jit::lookup(ctx->device, ctx->jit_vid, &k, &err, ctx->variant);
	if (st == ssx_jit::State::Ready) {
		std::swap(ctx->d_blob, ctx->d_blob_jit);
		ctx->blob_words = ctx->blob_jit_words; ctx->path_blob_words = ctx->path_blob_jit_words;
		ctx->topology = 3u;
		ctx->jit_kernels[ctx->variant] = k;
		ctx->resident_blocks = 0; ctx->gen_blocks = 0; // the blob's LDS footprint changed
		ctx->jit_pending = false; ctx->jit_state = SSX_JIT_STATE_SPECIALISED;
	} else if (st == ssx_jit::State::Failed) {
		ctx->jit_pending = false; ctx->jit_state = SSX_JIT_STATE_FAILED; ctx->jit_message = err;
	} else {
		ctx->generic_samples += samples;
		if (!ctx->jit_requested && ctx->generic_samples >= kJitAfterSamples) { ssx_jit::request(ctx->jit_vid, ctx->variant); ctx->jit_requested = true; }
	}
}

// A render in one libm of a scene that already runs on its own run-time compiled kernels (topology 3, its blob packed for them) but has
// only the other mode's: this mode's are compiled here, on the calling thread, the first time (or come from this process's memory / the disk
// cache: the mode is part of the pattern's key and of the compile flags, csrc/ssx_jit.h).  No fall-back: the generic kernels cannot read
// that blob.  Called before the context switches to `libm` (ready_to_launch): a failure leaves it in the mode it was in.
int ensure_libm_kernels(ssx_ctx* ctx, uint32_t libm) {
	const ssx_jit::Kernels*& have = ctx->jit_kernels[libm];
	if (ctx->topology != 3u || have) return SSX_OK;
	std::string err;
	const ssx_jit::Kernels* k = ssx_jit::get(ctx->device, ctx->jit_vid, &err, libm);
	if (!k) return fail(ctx, SSX_ERR_STATE, "the scene's specialised kernels for this libm could not be compiled: " + err);
	have = k;
	return SSX_OK;
}

// The context ready to launch a render with `p`: the kernels of its libm there and current (the plan of the resident workgroups is
// redone when the libm changes: the twins are different kernels), the pixel sums and -- asked for -- the output image sized.
int ready_to_launch(ssx_ctx* ctx, const ssx_render_params* p, bool need_out, bool keep_samples = false) {
	// spectral output on: the _flux twins (a specialised scene's are compiled here, on the calling thread, at its first spectral render).  They exist for the
	// default libm and spectral scenes only; the entry points refuse the rest while it is on (spectral_refuses)
	// A plain render of a plain scene: the _plain twins, likewise.  The choice is made here for every render, so a switch flipped on a context that has
	// rendered plain changes kernels (and the plan of the resident workgroups) at the next render.
	const uint32_t variant = variant_of(ctx, p, keep_samples);
	const int rc = ensure_libm_kernels(ctx, variant);
	if (rc) return rc;
	// (a scene still waiting for its own kernels asks again, for this mode's: maybe_swap_jit)
	ctx->libm = p->libm;
	if (ctx->variant != variant) { ctx->variant = variant; ctx->resident_blocks = 0; ctx->jit_requested = false; }
	SSX_HIP(ctx, ctx->d_accum.reserve(accum_bytes(p->width, p->height)));
	if (need_out) SSX_HIP(ctx, ctx->d_out.reserve(image_bytes(p->width, p->height)));
	return SSX_OK;
}

// samples [k0, k1) of every owned pixel, in stream order
int launch_range(ssx_ctx* ctx, LaunchPlan& pl, uint32_t k0, uint32_t k1, hipStream_t stream) {
	if (pl.args.my_tiles == 0 || k1 <= k0) return SSX_OK;
	Batch b = make_batch(ctx, pl, k0, k1);
	return launch_batch(ctx, b, stream);
}

// Samples [0,spp) in batches of `batch` spp, back to back on `stream`: the pixel sums continue from batch to batch
// (SsxKernelArgs::accum), the sample arrays and logs are reused.
int launch_batches(ssx_ctx* ctx, LaunchPlan& pl, uint32_t spp, uint32_t batch, hipStream_t stream) {
	for (uint32_t k0 = 0; k0 < spp; k0 += batch) {
		int rc = launch_range(ctx, pl, k0, (spp - k0 < batch) ? spp : k0 + batch, stream);
		if (rc) return rc;
	}
	return SSX_OK;
}

// A 64x64x4-sample render of the scene at upload time counts the continued levels per sample (plan_info: what the
// benchmark prices the algorithmic HBM bytes with, and what picks the unit size in make_batch).  It runs without the fold,
// so that st[] keeps the tail words, which are read back.
int calibrate(ssx_ctx* ctx) {
	ssx_render_params cp{};
	cp.struct_size = sizeof cp; cp.width = 64; cp.height = 64; cp.spp = 4; cp.tile_stride = 1;
	ctx->fuse_resolve = false; // no fold: st[] keeps {lambda_0, tail word, ...}, the level counts are read back below
	ctx->pre_hits = false;     // camera rays in the path loop: every ray that leaves the scene is counted there
	LaunchPlan pl = make_plan(ctx, &cp);
	int rc = ensure_samples(ctx, pl, cp.spp);
	if (rc) return rc;
	Batch b = make_batch(ctx, pl, 0, cp.spp);
	if (b.rc) return b.rc;
	// generate, then the calibration kernel: generic (it reads the per-quad vertex table: the whole blob is staged) with narrow queue entries
	if ((rc = enqueue_generate(ctx, b, ctx->stream))) return rc;
	const KernelRef kernel{ (const void*)ssx_calibrate_kernel };
	int blocks = 0;
	if ((rc = blocks_that_fit(ctx, kernel, path_lds_bytes(ctx->blob_words, SSX_QUEUE_WORDS_NARROW), &blocks))) return rc;
	if ((rc = enqueue_path(ctx, b, kernel, SSX_QUEUE_WORDS_NARROW, ctx->blob_words, blocks, ctx->stream))) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	std::vector<uint4> recs((size_t)b.n_rec);
	SSX_HIP(ctx, hipMemcpy(recs.data(), b.a.st, recs.size() * sizeof(uint4), hipMemcpyDeviceToHost));
	uint64_t frames = 0;
	for (const uint4& r : recs) frames += (r.y >> 2) & 0xFu;
	ctx->calib_frames = (float)((double)frames / (double)recs.size());
	uint32_t counters[2] = { 0u, 0u };
	SSX_HIP(ctx, hipMemcpy(counters, ctx->d_unit_counter.ptr, sizeof counters, hipMemcpyDeviceToHost));
	ctx->calib_left = (float)((double)counters[1] / (double)recs.size());
	// Tracing the camera rays ahead of the path loop (ssx_generate_kernel*) costs one coherent trace per sample (~650 wave
	// instructions per 64 samples) and saves, per ray that leaves the scene, the lane-iteration such a ray otherwise idles
	// through (a trace + a shading, ~2300 per 64 lanes): it pays from ~0.3 such rays per sample (Cornell box: 0.87; plane-srgb: 0).
	ctx->pre_hits = ctx->calib_left >= 0.3f;
	if (const char* e = debug_env("SSX_PRE_HITS")) { if (e[0] != '\0') ctx->pre_hits = e[0] != '0'; } // A/B runs and tests (an empty value changes nothing)
	ctx->fuse_resolve = true;
	// the waves' level logs for the unit size this scene renders with: allocated here, once (the device is idle)
	return ensure_logs(ctx, (unit_spp_of(ctx) + SSX_COHORT_KS - 1u) / SSX_COHORT_KS);
}

// `spp` = the samples per pixel actually accumulated (Options::spp, or fewer after ssx_render_stop)
int launch_finalize(ssx_ctx* ctx, const ssx_render_params* p, uint32_t spp, float* d_out, hipStream_t stream, uint32_t done_tiles = 0xFFFFFFFFu) {
	hipLaunchKernelGGL(ssx_finalize_kernel, pixel_blocks(p), dim3(256), 0, stream,
	                   ctx->d_accum.as<const double>(), (float4*)d_out, pixel_grid(p), spp, ctx->rgb_mode ? 1u : 0u, done_tiles);
	SSX_HIP(ctx, hipGetLastError());
	return SSX_OK;
}

// the noise estimate's part in the render loop (csrc/ssx_progressive.hip)
int noise_begin(ssx_ctx* ctx, const ssx_render_params* p, uint32_t k_begin, bool continuing);
int noise_batch(ssx_ctx* ctx, const ssx_render_params* p, uint32_t n_k, hipStream_t stream);
// ... and the spectral output's (csrc/ssx_spectral.hip)
int spectral_refuses(ssx_ctx* ctx, const ssx_render_params& p, bool tile_walk);
int spectral_begin(ssx_ctx* ctx, uint32_t my_tiles, bool continuing, bool* active);
int spectral_batch(ssx_ctx* ctx, const ssx_render_params* p, const LaunchPlan& pl, uint32_t n_k, hipStream_t stream);
// ... and the spectral moments' (csrc/ssx_spectral_stats.hip)
int moments_reserve(ssx_ctx* ctx, uint32_t my_tiles, bool continuing);
int moments_begin(ssx_ctx* ctx, uint32_t my_tiles, bool continuing, bool spectral, bool* active);
int moments_batch(ssx_ctx* ctx, const ssx_render_params* p, const LaunchPlan& pl, uint32_t n_k, hipStream_t stream);
void moments_publish(ssx_ctx* ctx, bool active);
void moments_invalidate(ssx_ctx* ctx, const char* why);
void moments_drop(ssx_ctx* ctx);

// The asynchronous render: one worker thread per call of ssx_render_start / ssx_render_continue, walking through the samples or the tiles.  The end
// of either walk: the image of what the sums hold, on the device, the stream idle.
int finish_walk(ssx_ctx* ctx, const ssx_render_params& p, uint32_t spp, uint32_t done_tiles) {
	if (const int rc = launch_finalize(ctx, &p, spp, ctx->d_out.as<float>(), ctx->stream, done_tiles)) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return SSX_OK;
}

// Samples per pixel of one launch of the sample walk over `span` samples: what the caller asked for, or 1/32 of the span raised to
// kSamplesPerSync per launch; never more than the sample arrays' budget allows.
uint32_t sample_walk_chunk(const ssx_render_params& p, uint32_t span, const LaunchPlan& pl) {
	const size_t pixels = (size_t)p.width * p.height;
	const uint64_t min_spp = kSamplesPerSync / (pixels ? pixels : 1) + 1u;
	uint32_t chunk = p.spp_per_launch ? p.spp_per_launch : (span + 31u) / 32u;
	if (!p.spp_per_launch && chunk < min_spp) chunk = (uint32_t)(min_spp < span ? min_spp : span);
	if (chunk == 0) chunk = 1;
	return chunk > pl.max_spp_per_launch ? pl.max_spp_per_launch : chunk;
}

// One launch of the tile walk: as many of the device's tiles as make kSamplesPerSync (at least one), all their samples -- in sample ranges of `spp` where one
// launch cannot hold them.  The sample arrays are sized by tiles x samples per launch: both are brought under the budget of make_plan (it assumed all tiles).
struct TileLaunch { uint32_t tiles, spp; };
TileLaunch tile_walk_launch(const ssx_render_params& p, const LaunchPlan& pl) {
	const uint32_t owned = pl.args.my_tiles;
	uint32_t spp_l = p.spp_per_launch ? p.spp_per_launch : p.spp;
	if (spp_l > p.spp) spp_l = p.spp;
	uint64_t per_launch = kSamplesPerSync / ((uint64_t)64 * p.spp) + 1u;
	if (const char* e = debug_env("SSX_TILES_PER_LAUNCH")) { const int v = atoi(e); if (v >= 1) per_launch = (uint64_t)v; } // tests (under SSX_DEBUG_ENV=1)
	if (per_launch > owned) per_launch = owned;
	const uint64_t budget_records = (uint64_t)pl.max_spp_per_launch * owned * 64u;
	while (spp_l > 1u && (uint64_t)spp_l * 64u > budget_records) spp_l = (spp_l + 1u) / 2u;
	const uint64_t fit = budget_records / ((uint64_t)spp_l * 64u);
	if (per_launch > fit) per_launch = fit ? fit : 1u;
	return TileLaunch{ (uint32_t)per_launch, spp_l };
}

// Every owned tile, sample range by sample range: samples [k_begin, p.spp) onto cleared sums, or (continuing: ssx_render_continue) onto the
// sums as they are.  A stop between two launches leaves every pixel at the same count.
int render_sample_walk(ssx_ctx* ctx, const ssx_render_params& p, uint32_t k_begin, bool continuing) {
	int rc;
	if (!continuing && (rc = clear_sums(ctx, p.width, p.height, ctx->stream))) return rc;
	if ((rc = noise_begin(ctx, &p, k_begin, continuing))) return rc;
	maybe_swap_jit(ctx, 0); // (the scene's own kernels, if they have arrived: the plan is of the blob that is current now)
	if ((rc = moments_reserve(ctx, owned_tiles(p), continuing))) return rc; // (before the plan asks the device for its free memory)
	LaunchPlan pl = make_plan(ctx, &p);
	bool spectral = false, moments = false;
	if ((rc = spectral_begin(ctx, pl.args.my_tiles, continuing, &spectral))) return rc;
	if ((rc = moments_begin(ctx, pl.args.my_tiles, continuing, spectral, &moments))) return rc;
	const uint32_t span = p.spp - k_begin, chunk = sample_walk_chunk(p, span, pl);
	if ((rc = ensure_samples(ctx, pl, chunk < span ? chunk : span))) return rc;
	for (uint32_t k0 = k_begin; k0 < p.spp && !ctx->stop_flag.load(); k0 += chunk) {
		const uint32_t k1 = (p.spp - k0 < chunk) ? p.spp : k0 + chunk;
		if (ctx->jit_pending) { // between launches the device is idle: the kernels may change here (same bits)
			maybe_swap_jit(ctx, (uint64_t)p.width * p.height * (k1 - k0) / p.tile_stride);
			if (!ctx->jit_pending) { const uint32_t cap = pl.max_spp_per_launch; pl = make_plan(ctx, &p); pl.max_spp_per_launch = cap; }
		}
		if ((rc = launch_range(ctx, pl, k0, k1, ctx->stream))) return rc;
		if (ctx->noise_on && (rc = noise_batch(ctx, &p, k1 - k0, ctx->stream))) return rc;
		if (spectral && (rc = spectral_batch(ctx, &p, pl, k1 - k0, ctx->stream))) return rc;
		if (moments && (rc = moments_batch(ctx, &p, pl, k1 - k0, ctx->stream))) return rc;
		SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		ctx->done_spp.store(k1);
	}
	// like the reference's last worker (renderer.cpp:388-394) the image is produced even after a stop.  The reference then holds finished tiles next
	// to untouched ones; here every pixel holds the mean of the samples accumulated so far (divisor = samples done, not Options::spp), i.e. a noisier
	// image of the right brightness with alpha as after a full render.
	const uint32_t done = ctx->done_spp.load();
	if ((rc = finish_walk(ctx, p, done ? done : p.spp, 0xFFFFFFFFu))) return rc;
	ctx->done_tiles.store(pl.args.my_tiles);
	ctx->sums.spectral_valid = spectral; // (the bins of the launches that ran: exactly the samples the sums hold)
	if (!spectral) ctx->spectral_note = "the render that made these sums ran without them (it continued sums that had none)";
	moments_publish(ctx, moments);
	sums_publish(ctx, done);
	return SSX_OK;
}

// The reference's walk (src/renderer.cpp:340-409; ssx_render_params::tile_major): the device's tile list from its first tile upwards, a few tiles per
// launch, every tile to the full sample count; a stop between launches leaves finished tiles next to untouched ones.  Same units, same kernels, same bits
// -- only the order of the work differs.  It takes no batches of the noise estimate: its sums, once finished, are adopted as ONE by the continue that follows.
int render_tile_walk(ssx_ctx* ctx, const ssx_render_params& p) {
	int rc;
	if ((rc = clear_sums(ctx, p.width, p.height, ctx->stream))) return rc;
	maybe_swap_jit(ctx, 0);
	const LaunchPlan pl = make_plan(ctx, &p);
	const uint32_t owned = pl.args.my_tiles;
	const TileLaunch per = tile_walk_launch(p, pl);
	LaunchPlan sized = pl; sized.args.my_tiles = per.tiles;
	if ((rc = ensure_samples(ctx, sized, per.spp))) return rc;
	for (uint32_t j0 = 0; j0 < owned && !ctx->stop_flag.load(); j0 += per.tiles) {
		const uint32_t j1 = (owned - j0 < per.tiles) ? owned : j0 + per.tiles;
		maybe_swap_jit(ctx, (uint64_t)(j1 - j0) * 64u * p.spp);
		LaunchPlan part = make_plan(ctx, &p);
		part.args.tile_first = p.tile_first + p.tile_stride * j0; // the device's tiles j0 .. j1-1 of its list
		part.args.my_tiles = j1 - j0;
		if ((rc = launch_batches(ctx, part, p.spp, per.spp, ctx->stream))) return rc;
		SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		ctx->done_tiles.store(j1);
		ctx->done_spp.store((uint32_t)((uint64_t)p.spp * j1 / owned)); // (progress; the finished tiles hold all p.spp samples)
	}
	const uint32_t done = ctx->done_tiles.load();
	if ((rc = finish_walk(ctx, p, p.spp, done))) return rc;
	if (done == owned) sums_publish(ctx, p.spp); // finished: every owned pixel holds [0, spp); stopped: tiles at different counts, nothing to continue
	return SSX_OK;
}

// The worker thread of one call: ctx->cur, from sample k_begin on.  A continued render walks through the samples whatever cur.tile_major says.
int render_walk(ssx_ctx* ctx, const ssx_render_params p, uint32_t k_begin, bool continuing) { // (its own copy of the parameters)
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	return (p.tile_major && !continuing) ? render_tile_walk(ctx, p) : render_sample_walk(ctx, p, k_begin, continuing);
}
void worker_main(ssx_ctx* ctx, uint32_t k_begin, bool continuing) {
	const int rc = render_walk(ctx, ctx->cur, k_begin, continuing);
	if (rc) sums_invalidate(ctx); // (a continued render had valid sums until here)
	ctx->worker_rc = rc;
	ctx->rendering.store(0);
}

// The tail of ssx_render_start and ssx_render_continue, behind their own checks (the context's device current): `p` becomes ctx->cur and a
// worker renders samples [k_begin, p.spp) of it, total_spp of them (ssx_progress).
int start_worker(ssx_ctx* ctx, const ssx_render_params& p, uint32_t k_begin, bool continuing, uint32_t total_spp) {
	if (ctx->worker.joinable()) ctx->worker.join();
	if (const int rc = spectral_refuses(ctx, p, p.tile_major && !continuing)) return rc;
	if (const int rc = ready_to_launch(ctx, &p, true)) return rc;
	ctx->cur = p; ctx->total_spp = total_spp; ctx->k_begin = k_begin;
	if (!continuing) { sums_invalidate(ctx); ctx->done_spp.store(0); ctx->done_tiles.store(0); } // (the worker publishes the sums it leaves)
	ctx->sums.imported = ctx->sums.spectral_imported = false;
	ctx->stop_flag.store(0); ctx->worker_rc = 0;
	ctx->rendering.store(1);
	ctx->worker = std::thread(worker_main, ctx, k_begin, continuing);
	return SSX_OK;
}

// ssx_scene_digest: the scene's tables packed without device addresses (no texel or table pointers: the same words in every process),
// then the uplift's table and the texels as the caller described them.  Eight bytes at a time through the splitmix64 finaliser.
uint64_t digest_mix(uint64_t h, uint64_t w) {
	uint64_t z = (h ^ w) + 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
uint64_t digest_bytes(uint64_t h, const void* data, size_t n) {
	const uint8_t* p = static_cast<const uint8_t*>(data);
	h = digest_mix(h, (uint64_t)n);
	for (; n >= 8; n -= 8, p += 8) { uint64_t w; memcpy(&w, p, 8); h = digest_mix(h, w); }
	if (n) { uint64_t w = 0; memcpy(&w, p, n); h = digest_mix(h, w); }
	return h;
}
uint64_t scene_digest_of(const ssx_scene_desc* s) {
	std::vector<uint32_t> blob;
	std::string err;
	const std::vector<const void*> no_tex(s->n_textures, nullptr);
	if (pack_blob(s, no_tex, nullptr, blob, err) != SSX_OK) return 0;
	uint64_t h = digest_bytes(0x5353584449474553ull, blob.data(), blob.size() * 4);
	for (uint32_t i = 0; i < s->n_textures; ++i) h = digest_bytes(h, s->textures[i].rgb, (size_t)3 * s->textures[i].width * s->textures[i].height);
	if (s->uplift == SSX_UPLIFT_JH) h = digest_bytes(h, s->jh_data, (size_t)3 * s->jh_res * s->jh_res * s->jh_res * 3 * sizeof(float));
	if (s->uplift == SSX_UPLIFT_MENG) {
		const ssx_meng_grid* g = s->meng;
		h = digest_bytes(h, g, offsetof(ssx_meng_grid, cells));
		h = digest_bytes(h, g->cells, (size_t)g->grid_w * g->grid_h * 32);
		h = digest_bytes(h, g->points, (size_t)g->n_points * (4 + (size_t)g->n_samples) * 4);
	}
	return h ? h : 1; // (0 means "no scene")
}

// the bounded, terminated copy of a text into a caller's buffer
void copy_text(const std::string& text, char* out, size_t out_size) {
	if (!out || !out_size) return;
	const size_t n = text.size() < out_size - 1 ? text.size() : out_size - 1;
	memcpy(out, text.data(), n); out[n] = '\0';
}

} // namespace

#include "ssx_rccl.h"

extern "C" {

int ssx_abi_version(void) { return SSX_ABI_VERSION; }

const char* ssx_last_error(const ssx_ctx* ctx) {
	if (!ctx) return g_create_error.c_str();
	ssx_ctx* c = const_cast<ssx_ctx*>(ctx);
	std::lock_guard<std::mutex> g(c->error_mutex);
	c->error_out = c->error;
	return c->error_out.c_str();
}

// The distinct libamdhip64 files mapped into the process ("a, b"): more than one means that somebody -- typically a Python process
// that loaded this library before torch without going through simple_spectral_amd/_capi.py -- brought a second HIP runtime, and
// streams / device pointers handed across the C ABI would belong to the other one.
static int mapped_hip_runtimes(std::string* names) {
	std::set<std::string> found;
	if (FILE* f = fopen("/proc/self/maps", "r")) {
		char line[4352];
		while (fgets(line, sizeof line, f)) {
			const char* path = strchr(line, '/');
			if (!path) continue;
			const char* base = strrchr(path, '/') + 1;
			if (strncmp(base, "libamdhip64.so", 14) != 0) continue;
			std::string p(path);
			while (!p.empty() && (p.back() == '\n' || p.back() == ' ')) p.pop_back();
			char real[PATH_MAX];
			found.insert(realpath(p.c_str(), real) ? std::string(real) : p);
		}
		fclose(f);
	}
	names->clear();
	for (const std::string& p : found) { if (!names->empty()) *names += ", "; *names += p; }
	return (int)found.size();
}

int ssx_create(int device, ssx_ctx** out) {
	if (!out) { g_create_error = "out is NULL"; return SSX_ERR_ARG; }
	*out = nullptr;
	{
		std::string names;
		if (mapped_hip_runtimes(&names) > 1) {
			g_create_error = "two HIP runtimes are mapped into this process (" + names + "): the hip_stream and device pointers of this interface must belong to "
			                 "the runtime this library is bound to.  Load one runtime only (Python: import simple_spectral_amd before, or together with, torch)";
			return SSX_ERR_DEVICE;
		}
	}
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n == 0) {
		g_create_error = fmt("no HIP device available (%s); this library has no CPU path", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
		return SSX_ERR_DEVICE;
	}
	if (device < 0 || device >= n) { g_create_error = fmt("device %d out of range (0..%d)", device, n - 1); return SSX_ERR_ARG; }
	hipDeviceProp_t prop;
	if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) { g_create_error = hipGetErrorString(e); return SSX_ERR_DEVICE; }
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
		g_create_error = fmt("device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
		return SSX_ERR_DEVICE;
	}
	ssx_ctx* ctx = new ssx_ctx;
	ctx->device = device;
	ctx->n_cus = prop.multiProcessorCount;
	ctx->max_wave_slots = (uint32_t)ctx->n_cus * 16u;
	if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) {
		g_create_error = hipGetErrorString(e);
		delete ctx;
		return SSX_ERR_DEVICE;
	}
	*out = ctx;
	return SSX_OK;
}

void ssx_destroy(ssx_ctx* ctx) {
	if (!ctx) return;
	if (ctx->worker.joinable()) { ctx->stop_flag.store(1); ctx->worker.join(); }
	(void)hipSetDevice(ctx->device);
	if (ctx->rccl_comm) { std::lock_guard<std::mutex> g(rccl_api().mutex); drop_rccl_comm(ctx); }
	if (ctx->ev_device_done) (void)hipEventDestroy(ctx->ev_device_done);
	for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
	const hipStream_t stream = ctx->stream;
	delete ctx; // the buffers go with it: the worker has joined, the context's device is current
	if (stream) (void)hipStreamDestroy(stream);
}

int ssx_upload_scene(ssx_ctx* ctx, const ssx_scene_desc* s) {
	if (!ctx) return SSX_ERR_ARG;
	ssx_scene_desc local;
	bool have_cam_dir = true;
	if (s && (s->struct_size == offsetof(ssx_scene_desc, meng) || s->struct_size == offsetof(ssx_scene_desc, cam_dir))) { // caller built before the Meng / cam_dir fields existed
		memset(&local, 0, sizeof local);
		memcpy(&local, s, s->struct_size);
		local.struct_size = sizeof(ssx_scene_desc);
		have_cam_dir = false;
		s = &local;
	}
	if (!s || s->struct_size != sizeof(ssx_scene_desc)) return fail(ctx, SSX_ERR_ARG, "ssx_scene_desc.struct_size mismatch");
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	SSX_HIP(ctx, hipDeviceSynchronize());
	ctx->device_pending = false;
	ctx->d_textures.clear();
	ctx->have_scene = false;
	sums_invalidate(ctx); ctx->scene_digest = 0;
	ctx->guides_width = ctx->guides_height = 0; // (the guide buffers were the last scene's)
	ctx->abins_width = ctx->abins_height = 0;   // (and so were the albedo bins)
	for (uint32_t i = 0; i < s->n_textures && i < SSX_MAX_TEXTURES; ++i) {
		const ssx_texture& t = s->textures[i];
		if (!t.rgb || t.width == 0 || t.height == 0) return fail(ctx, SSX_ERR_DATA, "Could not load texture"); // material.cpp:15-18
		const size_t bytes = (size_t)3 * t.width * t.height;
		ctx->d_textures.emplace_back();
		SSX_HIP(ctx, ctx->d_textures.back().reserve(bytes));
		SSX_HIP(ctx, hipMemcpy(ctx->d_textures.back().ptr, t.rgb, bytes, hipMemcpyHostToDevice));
	}
	if (s->uplift != SSX_MODE_RGB && s->uplift != SSX_UPLIFT_OURS && s->uplift != SSX_UPLIFT_JH && s->uplift != SSX_UPLIFT_MENG)
		return fail(ctx, SSX_ERR_SCENE, "unsupported uplift variant (0 = RGB mode, 1 = basis, 2 = Meng et al., 3 = Jakob-Hanika)");
	ctx->rgb_mode = (s->uplift == SSX_MODE_RGB);
	ctx->scene_traits = scene_traits_of(s);
	ctx->d_jh_data.release();
	if (s->uplift == SSX_UPLIFT_MENG) {
		// device table: 16 header words, cells, points (layout documented at meng_uplift in ssx_kernels.hip)
		const ssx_meng_grid* g = s->meng;
		if (!g || !g->cells || !g->points || g->grid_w == 0 || g->grid_h == 0 || g->grid_w > 4096 || g->grid_h > 4096 ||
		    g->n_points == 0 || g->n_points > (1u << 20) || g->n_samples < 2 || g->n_samples > 4096 || !(g->sample_max > g->sample_min))
			return fail(ctx, SSX_ERR_DATA, "Meng grid missing or invalid");
		const size_t n_cells = (size_t)g->grid_w * g->grid_h;
		for (size_t c = 0; c < n_cells; ++c) {
			const int32_t* cell = g->cells + 8 * c;
			const int32_t inside = cell[0], num = cell[1];
			// what spectrum_xyz_to_p can read without leaving the tables (spectrum_grid.h:47-131)
			const bool shape_ok = inside ? (num == 4) : (num == 0 || (num >= 3 && num <= 6));
			if (!shape_ok) return fail(ctx, SSX_ERR_DATA, "Meng grid: cell with an unusable point count");
			for (int32_t k = 0; k < num; ++k) if (cell[2 + k] < 0 || (uint32_t)cell[2 + k] >= g->n_points) return fail(ctx, SSX_ERR_DATA, "Meng grid: point index out of range");
		}
		const size_t words = 16 + n_cells * 8 + (size_t)g->n_points * (4 + (size_t)g->n_samples);
		std::vector<uint32_t> tab(words, 0u);
		tab[0] = g->grid_w; tab[1] = g->grid_h; tab[2] = g->n_points; tab[3] = g->n_samples;
		memcpy(&tab[4], &g->sample_min, 4); memcpy(&tab[5], &g->sample_max, 4);
		memcpy(&tab[6], g->xy_to_uv, 24);
		memcpy(&tab[16], g->cells, n_cells * 32);
		memcpy(&tab[16 + n_cells * 8], g->points, (size_t)g->n_points * (4 + (size_t)g->n_samples) * 4);
		SSX_HIP(ctx, ctx->d_jh_data.reserve(words * 4));
		SSX_HIP(ctx, hipMemcpy(ctx->d_jh_data.ptr, tab.data(), words * 4, hipMemcpyHostToDevice));
	}
	if (s->uplift == SSX_UPLIFT_JH) {
		// rgb2spec_load returns NULL for a missing table and the reference then crashes (color.cpp:144,220)
		if (!s->jh_scale || !s->jh_data || s->jh_res < 2 || s->jh_res > 256) return fail(ctx, SSX_ERR_DATA, "Jakob-Hanika model missing or invalid");
		size_t bytes = (size_t)3 * s->jh_res * s->jh_res * s->jh_res * 3 * sizeof(float);
		SSX_HIP(ctx, ctx->d_jh_data.reserve(bytes));
		SSX_HIP(ctx, hipMemcpy(ctx->d_jh_data.ptr, s->jh_data, bytes, hipMemcpyHostToDevice));
	}
	std::vector<uint32_t> blob, blob_jit;
	for (auto& k : ctx->jit_kernels) k = nullptr;
	ctx->jit_pending = ctx->jit_requested = false; ctx->generic_samples = 0; ctx->jit_vid.clear();
	ctx->jit_state = SSX_JIT_STATE_NONE; ctx->jit_message.clear();
	ctx->d_blob_jit.release();
	std::vector<const void*> tex;
	for (const DeviceBuffer& t : ctx->d_textures) tex.push_back(t.ptr);
	PackInfo info;
	std::string pack_err;
	int rc = pack_blob(s, tex, ctx->d_jh_data.ptr, blob, pack_err, -1, &info);
	if (rc) return fail(ctx, rc, pack_err);
	// A scene whose corners coincide in no built-in pattern: kernels specialised to ITS pattern (csrc/ssx_jit.h) -- from this
	// process's memory or the disk cache at once; else compiled here (mode 1) or by the background thread later (mode 2), the
	// generic kernel serving meanwhile.  A failure of any kind leaves the scene on the generic kernel: same bits.
	const int jit_mode = env_on("SSX_JIT_PASS1") ? SSX_JIT_AT_UPLOAD : ctx->jit_mode;
	// The kernels looked for (and, asked for at upload, compiled) here are those a render with default parameters will run: the scene's _plain twins if
	// its traits allow them.  A render with other switches gets its own at its start (ensure_libm_kernels), as a glibc-mode render does.  The context's
	// variant follows, unless its last render chose glibc mode or spectral output: what the introspection calls report until the next render decides again.
	ssx_render_params defaults{};
	const uint32_t upload_variant = variant_of(ctx, &defaults) == ssx_jit::kVariantPlain ? (uint32_t)ssx_jit::kVariantPlain : (uint32_t)SSX_LIBM_BUILD;
	if (ctx->variant == SSX_LIBM_BUILD || ctx->variant == ssx_jit::kVariantPlain) ctx->variant = upload_variant;
	if (info.candidate && jit_mode != SSX_JIT_OFF) {
		std::string err;
		const ssx_jit::Kernels* k = nullptr;
		ssx_jit::State st = ssx_jit::lookup(ctx->device, info.vid, &k, &err, upload_variant);
		if (st != ssx_jit::State::Ready && st != ssx_jit::State::Failed && jit_mode == SSX_JIT_AT_UPLOAD) {
			k = ssx_jit::get(ctx->device, info.vid, &err, upload_variant);
			st = k ? ssx_jit::State::Ready : ssx_jit::State::Failed;
		}
		if (st == ssx_jit::State::Failed) { ctx->jit_state = SSX_JIT_STATE_FAILED; ctx->jit_message = err; }
		else if ((rc = pack_blob(s, tex, ctx->d_jh_data.ptr, blob_jit, pack_err, 3))) return fail(ctx, rc, pack_err);
		else if (st == ssx_jit::State::Ready) { blob.swap(blob_jit); blob_jit.clear(); ctx->jit_kernels[upload_variant] = k; ctx->jit_vid = info.vid; ctx->jit_state = SSX_JIT_STATE_SPECIALISED; }
		else { ctx->jit_pending = true; ctx->jit_vid = info.vid; ctx->jit_state = SSX_JIT_STATE_GENERIC_MEANWHILE; ctx->jit_requested = (st == ssx_jit::State::Pending); }
	}
	if (ctx->jit_pending) {
		SSX_HIP(ctx, ctx->d_blob_jit.reserve(blob_jit.size() * 4));
		SSX_HIP(ctx, hipMemcpy(ctx->d_blob_jit.ptr, blob_jit.data(), blob_jit.size() * 4, hipMemcpyHostToDevice));
		const SsxBlobHeader* bh = reinterpret_cast<const SsxBlobHeader*>(blob_jit.data());
		ctx->blob_jit_words = (uint32_t)blob_jit.size(); ctx->path_blob_jit_words = bh->words_without_perm;
	}
	SSX_HIP(ctx, ctx->d_blob.reserve(blob.size() * 4));
	SSX_HIP(ctx, hipMemcpy(ctx->d_blob.ptr, blob.data(), blob.size() * 4, hipMemcpyHostToDevice));
	ctx->blob_words = (uint32_t)blob.size();
	{
		SsxBlobHeader* bh = reinterpret_cast<SsxBlobHeader*>(blob.data());
		ctx->topology = bh->topology;
		ctx->path_blob_words = (bh->topology || bh->perm_hbm) ? bh->words_without_perm : ctx->blob_words;
		if (bh->perm_hbm) { // the permuted vertex table is read from this copy (large scenes): tell the kernels where it is
			const uint64_t at = (uint64_t)(uintptr_t)(ctx->d_blob.as<uint32_t>() + bh->off_perm);
			bh->perm_ptr_lo = (uint32_t)at; bh->perm_ptr_hi = (uint32_t)(at >> 32);
			SSX_HIP(ctx, hipMemcpy(ctx->d_blob.ptr, blob.data(), sizeof(SsxBlobHeader), hipMemcpyHostToDevice));
			ctx->blob_words = bh->words_without_perm; // ... and stage only what precedes it
		}
	}
	ctx->have_cam_dir = have_cam_dir;
	ctx->lambda_min = s->lambda_min; ctx->lambda_step = s->lambda_step;
	ctx->n_quads = s->n_quads;
	ctx->resident_blocks = 0; ctx->gen_blocks = 0; // depend on the blob's LDS footprint
	ctx->have_scene = true;
	ctx->scene_digest = scene_digest_of(s);
	return calibrate(ctx);
}

// samples per pixel of one launch of ssx_render_device: what the caller asked for, or the whole render; where the sample arrays' budget
// allows less, launches of EQUAL size (plane-srgb 1024^2 at 1024 spp ran as 341 + 341 + 341 + 1 before round 6: a launch of one sample
// per pixel at the end of every render)
static uint32_t device_batch(const ssx_render_params* p, const LaunchPlan& pl) {
	uint32_t batch = p->spp_per_launch ? p->spp_per_launch : p->spp;
	if (batch > p->spp) batch = p->spp;
	if (batch > pl.max_spp_per_launch) {
		const uint32_t n = (p->spp + pl.max_spp_per_launch - 1u) / pl.max_spp_per_launch;
		batch = (p->spp + n - 1u) / n;
	}
	return batch;
}

int ssx_render_device(ssx_ctx* ctx, const ssx_render_params* p_in, void* d_xyza_out, void* hip_stream) {
	if (!ctx) return SSX_ERR_ARG;
	ssx_render_params pp;
	int rc = take_params(ctx, p_in, &pp);
	if (rc) return rc;
	const ssx_render_params* const p = &pp;
	if (!d_xyza_out) return fail(ctx, SSX_ERR_ARG, "d_xyza_out is NULL");
	if (ctx->spectral_bins) return fail(ctx, SSX_ERR_ARG, "spectral output is on (ssx_set_spectral_bins): ssx_render_device does not bin its samples; use ssx_render_start");
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "asynchronous render in progress");
	hipStream_t stream = (hipStream_t)hip_stream;
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	// the context's accumulators and per-sample arrays are shared by all renders: a render still queued by an
	// earlier call (possibly on another stream) has to finish first.  Stream-ordered, no host wait -- unless
	// a buffer has to grow, which frees the old one.
	if (!ctx->ev_device_done) SSX_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_device_done, hipEventDisableTiming));
	// The call may be recorded into a hipGraph (the stream is capturing): then nothing outside the capture can be waited for or
	// signalled from here -- an earlier render of this context must have completed, the buffers must have their size (render once
	// outside the capture first), and ordering the graph's replays against other uses of the context is the caller's business.
	hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
	(void)hipStreamIsCapturing(stream, &capture);
	const bool capturing = capture == hipStreamCaptureStatusActive;
	if (ctx->device_pending && capturing) return fail(ctx, SSX_ERR_STATE, "a render of this context may still be queued: ssx_render_device_wait before capturing another into a graph");
	// (the kernels of another libm may need a compilation and change the plan of the resident workgroups: not while capturing)
	if (capturing && ctx->variant != variant_of(ctx, p)) return fail(ctx, SSX_ERR_STATE, "ssx_render_params.libm differs from the context's last render: run it once outside the stream capture first");
	if (ctx->device_pending) SSX_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_device_done, 0));
	{
		LaunchPlan probe = make_plan(ctx, p, !capturing);
		// the batch ensure_samples below will size the arrays for -- the same expression.  While capturing the device cannot be asked
		// for its free memory and no buffer may grow: a launch may cover what the sample arrays of the warm-up render hold (cap_to_allocation).
		if (capturing) cap_to_allocation(ctx, probe);
		const uint32_t probe_batch = device_batch(p, probe);
		const size_t need = (size_t)probe.args.my_tiles * 64u * probe_batch;
		const bool grow = ctx->d_accum.bytes < accum_bytes(p->width, p->height) || ctx->d_samples.bytes < sample_bytes(ctx, need);
		if (grow && capturing) return fail(ctx, SSX_ERR_STATE, "the context's buffers have to grow for this render: run it once outside the stream capture first");
		if (grow && (rc = wait_device_pending(ctx))) return rc;
	}
	if ((rc = ready_to_launch(ctx, p, false))) return rc;
	sums_invalidate(ctx); // the sums become this render's, which is not continued
	if ((rc = clear_sums(ctx, p->width, p->height, stream))) return rc;
	if (!capturing) maybe_swap_jit(ctx, (uint64_t)p->width * p->height * p->spp / p->tile_stride);
	LaunchPlan pl = make_plan(ctx, p, !capturing);
	if (capturing) cap_to_allocation(ctx, pl);
	// one batch when the whole render fits the buffer budget, else batches back to back
	const uint32_t batch = device_batch(p, pl);
	if ((rc = ensure_samples(ctx, pl, batch))) return rc;
	if ((rc = launch_batches(ctx, pl, p->spp, batch, stream))) return rc;
	if ((rc = launch_finalize(ctx, p, p->spp, (float*)d_xyza_out, stream))) return rc;
	if (!capturing) {
		SSX_HIP(ctx, hipEventRecord(ctx->ev_device_done, stream));
		ctx->device_pending = true;
	}
	return SSX_OK;
}

int ssx_render_device_wait(ssx_ctx* ctx) {
	if (!ctx) return SSX_ERR_ARG;
	if (!ctx->device_pending) return SSX_OK;
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	return wait_device_pending(ctx);
}

int ssx_render_start(ssx_ctx* ctx, const ssx_render_params* p_in) {
	if (!ctx) return SSX_ERR_ARG;
	ssx_render_params pp;
	int rc = begin_render(ctx, p_in, &pp, "render already in progress");
	if (rc) return rc;
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if ((rc = wait_device_pending(ctx))) return rc;
	return start_worker(ctx, pp, 0, false, pp.spp);
}

int ssx_render_stop(ssx_ctx* ctx) {
	if (!ctx) return SSX_ERR_ARG;
	ctx->stop_flag.store(1);
	return SSX_OK;
}

int ssx_is_rendering(ssx_ctx* ctx) { return ctx ? ctx->rendering.load() : 0; }

float ssx_progress(ssx_ctx* ctx) {
	if (!ctx || ctx->total_spp == 0) return 0.0f;
	const uint32_t done = ctx->done_spp.load(); // (a continued render: this call's fraction)
	return done > ctx->k_begin ? (float)(done - ctx->k_begin) / (float)ctx->total_spp : 0.0f;
}

uint32_t ssx_done_spp(ssx_ctx* ctx) { return ctx ? ctx->done_spp.load() : 0u; }

uint32_t ssx_done_tiles(ssx_ctx* ctx) { return ctx ? ctx->done_tiles.load() : 0u; }

int ssx_render_wait(ssx_ctx* ctx, float* xyza_out) {
	if (!ctx) return SSX_ERR_ARG;
	if (!ctx->worker.joinable()) return fail(ctx, SSX_ERR_STATE, "no render was started");
	ctx->worker.join();
	if (ctx->worker_rc) return ctx->worker_rc;
	if (xyza_out) {
		SSX_HIP(ctx, hipSetDevice(ctx->device));
		SSX_HIP(ctx, hipMemcpy(xyza_out, ctx->d_out.ptr, image_bytes(ctx->cur.width, ctx->cur.height), hipMemcpyDeviceToHost));
	}
	return SSX_OK;
}

int ssx_set_timing(ssx_ctx* ctx, int enable) {
	if (!ctx) return SSX_ERR_ARG;
	ctx->timing = enable != 0;
	for (float& m : ctx->stage_ms) m = 0;
	ctx->ev_used = 0;
	return SSX_OK;
}

int ssx_get_timing(ssx_ctx* ctx, float stage_ms[4]) {
	if (!ctx || !stage_ms) return SSX_ERR_ARG;
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	int rc = collect_timing(ctx);
	if (rc) return rc;
	for (int k = 0; k < 4; ++k) { stage_ms[k] = ctx->stage_ms[k]; ctx->stage_ms[k] = 0; }
	return SSX_OK;
}

int ssx_read_framebuffer(ssx_ctx* ctx, float* xyza_out) {
	if (!ctx || !xyza_out) return SSX_ERR_ARG;
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	if (!ctx->d_out.ptr || ctx->cur.width == 0) return fail(ctx, SSX_ERR_STATE, "no render was started");
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	SSX_HIP(ctx, hipMemcpy(xyza_out, ctx->d_out.ptr, image_bytes(ctx->cur.width, ctx->cur.height), hipMemcpyDeviceToHost));
	return SSX_OK;
}

void* ssx_device_framebuffer(ssx_ctx* ctx) { return ctx ? ctx->d_out.ptr : nullptr; }

int ssx_device_index(ssx_ctx* ctx) { return ctx ? ctx->device : -1; }

int ssx_accumulate_peer(ssx_ctx* ctx, void* d_dst, int src_device, const void* d_src, uint32_t width, uint32_t height, void* hip_stream) {
	if (!ctx || !d_dst || !d_src || width == 0 || height == 0) return SSX_ERR_ARG;
	hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	const size_t pixels = (size_t)width * height, bytes = image_bytes(width, height);
	SSX_HIP(ctx, ctx->d_peer.reserve(bytes));
	if (src_device != ctx->device) {
		int can = 0;
		SSX_HIP(ctx, hipDeviceCanAccessPeer(&can, ctx->device, src_device));
		if (can) { hipError_t e = hipDeviceEnablePeerAccess(src_device, 0); if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) SSX_HIP(ctx, e); (void)hipGetLastError(); }
	}
	// device-to-device over xGMI (the runtime stages through the host only when peer access is unavailable)
	SSX_HIP(ctx, hipMemcpyPeerAsync(ctx->d_peer.ptr, ctx->device, d_src, src_device, bytes, stream));
	hipLaunchKernelGGL(ssx_sum_kernel, dim3((uint32_t)((pixels + 255u) / 256u)), dim3(256), 0, stream, (float4*)d_dst, ctx->d_peer.as<const float4>(), (uint32_t)pixels);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(stream));
	return SSX_OK;
}

// ---- diagnostics for the parity tests (never called during a normal render) ----------------------

int ssx_debug_eval(ssx_ctx* ctx, uint32_t op, const void* in, uint32_t in_words, void* out, uint32_t out_words, uint32_t n) {
	if (!ctx || !in || !out || in_words == 0 || out_words == 0 || out_words > 12u || n == 0) return SSX_ERR_ARG;
	if (!ctx->have_scene) return fail(ctx, SSX_ERR_STATE, "no scene uploaded");
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	DeviceBuffer d_in, d_out;
	SSX_HIP(ctx, d_in.reserve((size_t)n * in_words * 4));
	if (d_out.reserve((size_t)n * out_words * 4) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, SSX_ERR_DEVICE, "out of device memory (ssx_debug_eval)"); }
	SSX_HIP(ctx, hipMemcpy(d_in.ptr, in, (size_t)n * in_words * 4, hipMemcpyHostToDevice));
	SsxKernelArgs a{};
	a.blob = ctx->d_blob.as<uint32_t>(); a.blob_words = ctx->blob_words; a.rgb_mode = ctx->rgb_mode ? 1u : 0u;
	const size_t lds = staged_blob_lds(ctx->blob_words);
	if (op == SSX_DBG_TRACE_MASKED && in_words < 11u) return fail(ctx, SSX_ERR_ARG, "SSX_DBG_TRACE_MASKED: a row is orig[3], dir[3], ignore, mask[4]");
	if (op == SSX_DBG_TRACE_TOPO) {
		// the trace of the context's topology, in a kernel of its own (csrc/ssx_debug.hip); a scene on its own pattern's kernels gets the debug-only
		// variant of its run-time program, compiled -- or found in memory / on disk -- at the first call (csrc/ssx_jit.h kVariantDebug)
		if (in_words < 8u) return fail(ctx, SSX_ERR_ARG, "SSX_DBG_TRACE_TOPO: a row is orig[3], dir[3], ignore, has_ray");
		if (ctx->topology == 0u) return fail(ctx, SSX_ERR_STATE, "SSX_DBG_TRACE_TOPO: the context runs the generic trace (topology 0); that is SSX_DBG_TRACE");
		const uint32_t* d_rows = d_in.as<uint32_t>(); uint32_t* d_res = d_out.as<uint32_t>();
		void* args[] = { &a, &d_rows, &in_words, &d_res, &out_words, &n };
		if (ctx->topology == 3u) {
			std::string err;
			const ssx_jit::Kernels* k = ssx_jit::get(ctx->device, ctx->jit_vid, &err, ssx_jit::kVariantDebug);
			if (!k || !k->debug_trace) return fail(ctx, SSX_ERR_STATE, "SSX_DBG_TRACE_TOPO: the debug kernel of the scene's pattern could not be compiled: " + err);
			SSX_HIP(ctx, hipModuleLaunchKernel(k->debug_trace, (n + 255u) / 256u, 1, 1, 256, 1, 1, (unsigned)lds, ctx->stream, args, nullptr));
		} else {
			const void* host = ctx->topology == 1u ? (const void*)ssx_debug_trace_cornell_kernel : (const void*)ssx_debug_trace_plane_kernel;
			SSX_HIP(ctx, hipLaunchKernel(host, dim3((n + 255u) / 256u), dim3(256), args, lds, ctx->stream));
		}
		SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		SSX_HIP(ctx, hipMemcpy(out, d_out.ptr, (size_t)n * out_words * 4, hipMemcpyDeviceToHost));
		return SSX_OK;
	}
	const auto kernel =op >= SSX_DBG_GLIBC_MATH && op <= SSX_DBG_COSHEMI_GLIBC ? ssx_debug_eval_glibc_kernel : ssx_debug_eval_kernel; // the units of libm = glibc-2.35: a kernel that stages the _glibc kernels' LDS table
	hipLaunchKernelGGL(kernel, dim3((n + 255u) / 256u), dim3(256), lds, ctx->stream, a, op, d_in.as<uint32_t>(), in_words, d_out.as<uint32_t>(), out_words, n);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(out, d_out.ptr, (size_t)n * out_words * 4, hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_debug_sweep(ssx_ctx* ctx, uint32_t op, uint32_t lo, uint64_t count, uint64_t result[11]) {
	if (!ctx || !result || count == 0 || count > (1ull << 32)) return SSX_ERR_ARG;
	if (!ctx->have_scene) return fail(ctx, SSX_ERR_STATE, "no scene uploaded");
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	DeviceBuffer d_res;
	SSX_HIP(ctx, d_res.reserve(11 * sizeof(unsigned long long)));
	SSX_HIP(ctx, hipMemsetAsync(d_res.ptr, 0, 11 * sizeof(unsigned long long), ctx->stream));
	SsxKernelArgs a{};
	a.blob = ctx->d_blob.as<uint32_t>(); a.blob_words = ctx->blob_words;
	const size_t lds = staged_blob_lds(ctx->blob_words);
	const auto kernel = op >= SSX_SWEEP_GLIBC_SIN ? ssx_debug_sweep_glibc_kernel : ssx_debug_sweep_kernel; // libm = glibc-2.35 (see ssx_debug_eval)
	hipLaunchKernelGGL(kernel, dim3(256 * 16), dim3(256), lds, ctx->stream, a, op, lo, (uint64_t)count, d_res.as<unsigned long long>());
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(result, d_res.ptr, 11 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	return SSX_OK;
}

int ssx_debug_samples(ssx_ctx* ctx, const ssx_render_params* p_in, float* xyza, uint64_t* rng_state, uint32_t* levels) {
	if (!ctx) return SSX_ERR_ARG;
	ssx_render_params pp;
	int rc = begin_render(ctx, p_in, &pp, "render in progress");
	if (rc) return rc;
	const ssx_render_params* const p = &pp;
	if (p->tile_first != 0 || p->tile_stride != 1) return fail(ctx, SSX_ERR_ARG, "ssx_debug_samples renders the whole image");
	if ((rc = spectral_refuses(ctx, pp, false))) return rc;
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if ((rc = wait_device_pending(ctx))) return rc;
	if ((rc = ready_to_launch(ctx, p, false, true))) return rc; // (keep_samples below: the general kernels)
	LaunchPlan pl = make_plan(ctx, p);
	if (p->spp > pl.max_spp_per_launch) return fail(ctx, SSX_ERR_ARG, "ssx_debug_samples: too many samples for one launch");
	if ((rc = ensure_samples(ctx, pl, p->spp))) return rc;
	sums_invalidate(ctx);
	if ((rc = clear_sums(ctx, p->width, p->height, ctx->stream))) return rc;
	Batch b = make_batch(ctx, pl, 0, p->spp);
	b.a.keep_samples = 1u; // the fold leaves every sample's {X, Y, Z, alpha} in ray[]
	if ((rc = launch_batch(ctx, b, ctx->stream))) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	std::vector<float4> ray((size_t)b.n_rec);
	std::vector<uint4> st((size_t)b.n_rec);
	SSX_HIP(ctx, hipMemcpy(ray.data(), b.a.ray, ray.size() * sizeof(float4), hipMemcpyDeviceToHost));
	SSX_HIP(ctx, hipMemcpy(st.data(), b.a.st, st.size() * sizeof(uint4), hipMemcpyDeviceToHost));
	const uint32_t spp = p->spp, tiles_x = tiles_across(p->width);
	for (uint32_t j = 0; j < p->height; ++j) for (uint32_t i = 0; i < p->width; ++i) {
		const uint32_t tile = (j >> 3) * tiles_x + (i >> 3), lane = (j & 7u) * 8u + (i & 7u);
		for (uint32_t k = 0; k < spp; ++k) {
			const size_t r = ((size_t)tile * spp + k) * 64u + lane, o = ((size_t)j * p->width + i) * spp + k;
			if (xyza) { xyza[4 * o + 0] = ray[r].x; xyza[4 * o + 1] = ray[r].y; xyza[4 * o + 2] = ray[r].z; xyza[4 * o + 3] = ray[r].w; }
			if (rng_state) rng_state[o] = ((uint64_t)st[r].w << 32) | st[r].z;
			if (levels) levels[o] = (st[r].y >> 2) & 0xFu;
		}
	}
	return SSX_OK;
}

// The tile masks of a render with these parameters: the launch plan as a render builds it (make_plan), ssx_tile_mask_kernel as enqueue_generate
// launches it, into a buffer of the call's own -- the context's sample arrays, sums and continuable state are not touched, and the scene need
// not be one whose camera rays are pre-traced.
int ssx_debug_tile_mask(ssx_ctx* ctx, const ssx_render_params* p_in, uint32_t* out) {
	if (!ctx || !out) return SSX_ERR_ARG;
	ssx_render_params pp;
	int rc = begin_render(ctx, p_in, &pp, "render in progress");
	if (rc) return rc;
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if ((rc = wait_device_pending(ctx))) return rc;
	const LaunchPlan pl = make_plan(ctx, &pp);
	SsxKernelArgs ga = pl.args;
	if (ga.my_tiles == 0u) return SSX_OK;
	ga.blob_words = ctx->blob_words;
	const size_t bytes = (size_t)ga.my_tiles * 4u * sizeof(uint32_t);
	DeviceBuffer d_mask;
	if (d_mask.reserve(bytes) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, SSX_ERR_DEVICE, "out of device memory (ssx_debug_tile_mask)"); }
	ga.tile_mask = d_mask.as<uint32_t>();
	hipLaunchKernelGGL(ssx_tile_mask_kernel, dim3((ga.my_tiles + 3u) / 4u), dim3(256), 0, ctx->stream, ga);
	SSX_HIP(ctx, hipGetLastError());
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(out, d_mask.ptr, bytes, hipMemcpyDeviceToHost));
	return SSX_OK;
}

// Samples [k0, k0 + n_k) of every owned pixel as the first stage of a render makes them: the launch plan of a render with these parameters (make_plan), then
// enqueue_generate itself -- ssx_tile_mask_kernel where camera rays are pre-traced, ssx_generate_kernel with the grid a render gives it -- on sample arrays and
// tile masks of the call's own, filled with SSX_GENERATE_FILL_BYTE beforehand: a word no lane wrote comes back as the fill.  No path kernel runs; the context's
// sample arrays, sums and continuable state are not touched.  pre_hits: 0 / 1, or -1 for what the uploaded scene's calibration chose.
int ssx_debug_generate(ssx_ctx* ctx, const ssx_render_params* p_in, uint32_t k0, uint32_t n_k, int pre_hits, float* ray, uint32_t* st, float* hit) {
	if (!ctx || !ray || !st) return SSX_ERR_ARG;
	ssx_render_params pp;
	int rc = begin_render(ctx, p_in, &pp, "render in progress");
	if (rc) return rc;
	if (n_k == 0) return fail(ctx, SSX_ERR_ARG, "ssx_debug_generate: n_k must be positive");
	if ((uint64_t)k0 + n_k > 0xFFFFFFFFull) return fail(ctx, SSX_ERR_ARG, "ssx_debug_generate: k0 + n_k does not fit in 32 bits");
	if (pre_hits < -1 || pre_hits > 1) return fail(ctx, SSX_ERR_ARG, "ssx_debug_generate: pre_hits is 0, 1 or -1 (the context's own choice)");
	const bool pre = pre_hits < 0 ? ctx->pre_hits : pre_hits == 1;
	if (pre && !hit) return fail(ctx, SSX_ERR_ARG, "ssx_debug_generate: camera rays are pre-traced, hit must not be NULL");
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if ((rc = wait_device_pending(ctx))) return rc;
	const LaunchPlan pl = make_plan(ctx, &pp);
	if (n_k > pl.max_spp_per_launch) return fail(ctx, SSX_ERR_ARG, fmt("ssx_debug_generate: %u samples per pixel are more than one launch may cover (%u)", n_k, pl.max_spp_per_launch));
	Batch b{};
	b.a = pl.args;
	SsxKernelArgs& a = b.a;
	if (a.my_tiles == 0u) return SSX_OK;
	a.k0 = k0; a.k1 = k0 + n_k;
	a.n_records = (uint64_t)a.my_tiles * n_k * 64u;
	a.pre_hits = pre ? 1u : 0u;
	b.n_rec = a.n_records;
	const size_t rec_bytes = (size_t)a.n_records * 16u, mask_bytes = (size_t)a.my_tiles * 4u * sizeof(uint32_t);
	DeviceBuffer d_rec, d_mask;
	if (d_rec.reserve(3u * rec_bytes) != hipSuccess || d_mask.reserve(mask_bytes) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, SSX_ERR_DEVICE, "out of device memory (ssx_debug_generate)"); }
	SSX_HIP(ctx, hipMemsetAsync(d_rec.ptr, (int)SSX_GENERATE_FILL_BYTE, 3u * rec_bytes, ctx->stream));
	SSX_HIP(ctx, hipMemsetAsync(d_mask.ptr, 0, mask_bytes, ctx->stream));
	a.ray = reinterpret_cast<float4*>(d_rec.as<uint8_t>());
	a.st = reinterpret_cast<uint4*>(d_rec.as<uint8_t>() + rec_bytes);
	a.hit = reinterpret_cast<float4*>(d_rec.as<uint8_t>() + 2u * rec_bytes);
	a.tile_mask = d_mask.as<uint32_t>();
	if ((rc = enqueue_generate(ctx, b, ctx->stream))) return rc;
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(ray, a.ray, rec_bytes, hipMemcpyDeviceToHost));
	SSX_HIP(ctx, hipMemcpy(st, a.st, rec_bytes, hipMemcpyDeviceToHost));
	if (hit) SSX_HIP(ctx, hipMemcpy(hit, a.hit, rec_bytes, hipMemcpyDeviceToHost));
	return SSX_OK;
}

// The fold on the caller's levels (csrc/ssx_debug.hip debug_fold_body): the twin a render of this context with these parameters runs -- queue entries as
// pick_queue finds them for that render's path kernel, its libm, its _flux twin while spectral output is on -- in buffers of the call's own: sample arrays,
// level logs and sums.  Neither the context's arrays nor its libm, plan or continuable state are touched.
int ssx_debug_fold(ssx_ctx* ctx, const ssx_render_params* p_in, uint32_t n_pixels, uint32_t spp, const uint32_t* levels, uint32_t order_seed, uint32_t parked,
                   float* out_flux, float* out_xyza, double* out_sums) {
	if (!ctx || !levels) return SSX_ERR_ARG;
	ssx_render_params pp;
	int rc = begin_render(ctx, p_in, &pp, "render in progress");
	if (rc) return rc;
	if (n_pixels == 0 || (n_pixels & 63u) || n_pixels > (1u << 20)) return fail(ctx, SSX_ERR_ARG, "ssx_debug_fold: n_pixels must be a multiple of 64, at most 2^20");
	if (spp == 0 || spp > SSX_MAX_UNIT_KS) return fail(ctx, SSX_ERR_ARG, "ssx_debug_fold: spp must be 1..8, the samples per pixel of a work unit");
	if (parked > 1u) return fail(ctx, SSX_ERR_ARG, "ssx_debug_fold: parked is 0 or 1");
	const bool flux = ctx->spectral_bins && pp.libm == SSX_LIBM_BUILD && !ctx->rgb_mode; // (ready_to_launch)
	if (ctx->spectral_bins && !flux) return fail(ctx, SSX_ERR_STATE, "ssx_debug_fold: spectral output is on, and it renders spectral scenes with the default libm only");
	if (out_flux && !flux) return fail(ctx, SSX_ERR_STATE, "ssx_debug_fold: out_flux needs spectral output (ssx_set_spectral_bins)");
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if ((rc = wait_device_pending(ctx))) return rc;
	// the queue entries of that render's path kernel (pick_queue looks at the kernels of ctx->variant: lent for the question, and put back)
	const uint32_t variant = flux ? (uint32_t)ssx_jit::kVariantFlux : pp.libm, variant_was = ctx->variant;
	uint32_t qw = 0;
	ctx->variant = variant;
	rc = pick_queue(ctx, ctx->path_blob_words, &qw, nullptr);
	ctx->variant = variant_was;
	if (rc) return rc;
	const bool narrow = qw == SSX_QUEUE_WORDS_NARROW;
	const uint32_t n_tiles = n_pixels / 64u, cohorts = (spp + SSX_COHORT_KS - 1u) / SSX_COHORT_KS;
	const size_t n_rec = (size_t)n_pixels * spp, log_records = (size_t)n_tiles * 2u * cohorts * SSX_COHORT_RECORDS;
	const size_t row_bytes = n_rec * SSX_FOLD_ROW_WORDS * 4u;
	// (the kernels address the logs with 32-bit byte offsets: ensure_logs)
	if (log_records * SSX_LOG_BYTES_PER_RECORD >= ((size_t)1 << 32)) return fail(ctx, SSX_ERR_ARG, "ssx_debug_fold: level logs beyond 4 GiB for this many pixels and samples; fold fewer pixels per call");
	DeviceBuffer d_rows, d_samples, d_logs, d_sums;
	if (d_rows.reserve(row_bytes) != hipSuccess || d_samples.reserve(n_rec * SSX_BYTES_PER_SAMPLE_FLUX) != hipSuccess ||
	    d_logs.reserve(log_records * SSX_LOG_BYTES_PER_RECORD) != hipSuccess || d_sums.reserve((size_t)n_tiles * 256u * sizeof(double)) != hipSuccess) {
		(void)hipGetLastError();
		return fail(ctx, SSX_ERR_DEVICE, "out of device memory (ssx_debug_fold)");
	}
	SSX_HIP(ctx, hipMemcpy(d_rows.ptr, levels, row_bytes, hipMemcpyHostToDevice));
	SsxKernelArgs a{};
	a.blob = ctx->d_blob.as<uint32_t>(); a.blob_words = ctx->path_blob_words;
	a.rgb_mode = ctx->rgb_mode ? 1u : 0u;
	a.no_flat_field = pp.no_flat_field_correction ? 1u : 0u;
	a.keep_samples = 1u; // {X, Y, Z, alpha} of every sample stays in ray[]: where a parked sample waits, too
	a.unit_cohorts = cohorts; a.group_spp = spp; a.n_records = n_rec;
	bind_arrays(a, d_samples.as<uint8_t>(), n_rec, d_logs.as<uint8_t>(), log_records, flux);
	a.accum = d_sums.as<double>();
	static const void* const kFoldKernels[ssx_jit::kVariants][2] = {
		{ (const void*)ssx_debug_fold_kernel, (const void*)ssx_debug_fold_kernel_nq }, { (const void*)ssx_debug_fold_kernel_glibc, (const void*)ssx_debug_fold_kernel_nq_glibc },
		{ (const void*)ssx_debug_fold_kernel_flux, (const void*)ssx_debug_fold_kernel_nq_flux } };
	const uint32_t* d_in = d_rows.as<uint32_t>();
	void* args[] = { &a, &d_in, (void*)&n_tiles, &spp, &order_seed, &parked };
	const size_t lds = staged_blob_lds(a.blob_words) + 4u * SSX_WAVE_COUNTER_WORDS * 4u; // the four waves' hand-over words behind the blob, where the path kernel's queues begin
	SSX_HIP(ctx, hipLaunchKernel(kFoldKernels[variant][narrow], dim3((n_tiles + 3u) / 4u), dim3(256), args, lds, ctx->stream));
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	std::vector<float4> rec(n_rec);
	std::vector<double> sums((size_t)n_tiles * 256u);
	// device order [tile][k][pixel of the tile] -> the caller's [pixel][k]
	auto gather = [&](const void* d_src, float* out) -> int {
		SSX_HIP(ctx, hipMemcpy(rec.data(), d_src, n_rec * sizeof(float4), hipMemcpyDeviceToHost));
		for (uint32_t t = 0; t < n_tiles; ++t) for (uint32_t k = 0; k < spp; ++k) for (uint32_t l = 0; l < 64u; ++l)
			memcpy(out + 4u * (((size_t)t * 64u + l) * spp + k), &rec[((size_t)t * spp + k) * 64u + l], sizeof(float4));
		return SSX_OK;
	};
	if (out_flux && (rc = gather(a.flux, out_flux))) return rc;
	if (out_xyza && (rc = gather(a.ray, out_xyza))) return rc;
	if (out_sums) {
		SSX_HIP(ctx, hipMemcpy(sums.data(), d_sums.ptr, sums.size() * sizeof(double), hipMemcpyDeviceToHost));
		for (uint32_t t = 0; t < n_tiles; ++t) for (uint32_t l = 0; l < 64u; ++l) for (uint32_t c = 0; c < 4u; ++c)
			out_sums[((size_t)t * 64u + l) * 4u + c] = sums[(size_t)t * 256u + c * 64u + l];
	}
	return SSX_OK;
}

// One iteration of the path loop per round on the caller's paths (csrc/ssx_debug.hip debug_step_body): the twin a render of this context with these parameters
// runs -- its topology (0, 1, 2), the queue entries pick_queue finds for that render's path kernel, its libm -- in buffers of the call's own: rows, answers,
// sample records, level logs.  Every row is checked before anything is launched: what a row may index (its level's emission slot by depth, a quad's record
// by ignore, the tables by lambda_0) and what its words are packed into (prev_slot's 13 bits).
int ssx_debug_step(ssx_ctx* ctx, const ssx_render_params* p_in, uint32_t n_rows, uint32_t n_rounds, const uint32_t* rows, uint32_t* out) {
	if (!ctx || !rows || !out) return SSX_ERR_ARG;
	ssx_render_params pp;
	int rc = begin_render(ctx, p_in, &pp, "render in progress");
	if (rc) return rc;
	if (n_rounds == 0 || n_rounds > SSX_MAX_UNIT_KS) return fail(ctx, SSX_ERR_ARG, "ssx_debug_step: n_rounds must be 1..8, the samples per pixel of a work unit (SSX_COHORT_KS x unit_cohorts)");
	if (n_rows == 0 || (n_rows & 63u)) return fail(ctx, SSX_ERR_ARG, "ssx_debug_step: n_rows must be a multiple of 64");
	if (n_rows % (64u * n_rounds)) return fail(ctx, SSX_ERR_ARG, "ssx_debug_step: n_rows must be a multiple of 64 * n_rounds (whole tiles)");
	const uint32_t n_tiles = n_rows / (64u * n_rounds), cohorts = (n_rounds + SSX_COHORT_KS - 1u) / SSX_COHORT_KS;
	if (n_tiles > 65536u) return fail(ctx, SSX_ERR_ARG, "ssx_debug_step: n_rows is more than 65536 tiles of rows");
	const size_t log_records = (size_t)n_tiles * 2u * cohorts * SSX_COHORT_RECORDS;
	// (the kernels address the logs with 32-bit byte offsets: ensure_logs)
	if (log_records * SSX_LOG_BYTES_PER_RECORD >= ((size_t)1 << 32)) return fail(ctx, SSX_ERR_ARG, "ssx_debug_step: level logs beyond 4 GiB for this many rows; step fewer rows per call");
	if (ctx->topology > 2u) return fail(ctx, SSX_ERR_STATE, "ssx_debug_step: the context runs kernels compiled for its scene's own pattern (topology 3), which this op leaves out");
	if (pp.libm > 1u) return fail(ctx, SSX_ERR_STATE, "internal: ssx_debug_step with an unknown libm"); // (kStepKernels below has the two modes check_params lets through)
	const float lam_lo = ctx->rgb_mode ? 0.0f : ctx->lambda_min, lam_hi = ctx->rgb_mode ? 0.0f : ctx->lambda_min + ctx->lambda_step;
	for (uint32_t i = 0; i < n_rows; ++i) {
		const uint32_t* x = rows + (size_t)i * SSX_STEP_ROW_WORDS;
		float lam;
		memcpy(&lam, x + SSX_STEP_R_LAMBDA0, sizeof lam);
		const char* what = nullptr;
		if (x[SSX_STEP_R_DEPTH] >= SSX_MAX_DEPTH_) what = "depth must be below MAX_DEPTH (csrc/ssx_kernels.hip SSX_MAX_DEPTH_)";
		else if ((int32_t)x[SSX_STEP_R_IGNORE] != -1 && x[SSX_STEP_R_IGNORE] >= ctx->n_quads) what = "ignore must be -1 or a quad of the scene";
		else if (x[SSX_STEP_R_PREV_SLOT] > SSX_NO_SLOT) what = "prev_slot must be at most SSX_STEP_NO_SLOT";
		else if (!(lam >= lam_lo && lam <= lam_hi)) what = "lambda_0 must lie in the scene's [lambda_min, lambda_min + lambda_step] (0 in RGB mode)";
		if (what) return fail(ctx, SSX_ERR_ARG, fmt("ssx_debug_step: row %u: %s", i, what));
	}
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	if ((rc = wait_device_pending(ctx))) return rc;
	// the queue entries of that render's path kernel (pick_queue looks at the kernels of ctx->variant: lent for the question, and put back)
	const uint32_t variant = pp.libm, variant_was = ctx->variant;
	uint32_t qw = 0;
	ctx->variant = variant;
	rc = pick_queue(ctx, ctx->path_blob_words, &qw, nullptr);
	ctx->variant = variant_was;
	if (rc) return rc;
	const bool narrow = qw == SSX_QUEUE_WORDS_NARROW;
	const size_t row_bytes = (size_t)n_rows * SSX_STEP_ROW_WORDS * 4u, out_bytes = (size_t)n_rows * SSX_STEP_OUT_WORDS * 4u;
	DeviceBuffer d_rows, d_out, d_samples, d_logs;
	if (d_rows.reserve(row_bytes) != hipSuccess || d_out.reserve(out_bytes) != hipSuccess || d_samples.reserve((size_t)n_rows * SSX_BYTES_PER_SAMPLE) != hipSuccess ||
	    d_logs.reserve(log_records * SSX_LOG_BYTES_PER_RECORD) != hipSuccess) {
		(void)hipGetLastError();
		return fail(ctx, SSX_ERR_DEVICE, "out of device memory (ssx_debug_step)");
	}
	SSX_HIP(ctx, hipMemcpy(d_rows.ptr, rows, row_bytes, hipMemcpyHostToDevice));
	SSX_HIP(ctx, hipMemsetAsync(d_out.ptr, 0, out_bytes, ctx->stream));
	SsxKernelArgs a{};
	a.blob = ctx->d_blob.as<uint32_t>(); a.blob_words = ctx->path_blob_words;
	a.rgb_mode = ctx->rgb_mode ? 1u : 0u;
	a.indirect_only = pp.indirect_only ? 1u : 0u;
	a.no_els = pp.no_explicit_light_sampling ? 1u : 0u;
	a.unit_cohorts = cohorts; a.group_spp = n_rounds; a.n_records = n_rows;
	a.queue_words = qw;
	bind_arrays(a, d_samples.as<uint8_t>(), n_rows, d_logs.as<uint8_t>(), log_records, false);
	static const void* const kStepKernels[2][3][2] = {
		{ { (const void*)ssx_debug_step_kernel, (const void*)ssx_debug_step_kernel_nq }, { (const void*)ssx_debug_step_kernel_cornell, (const void*)ssx_debug_step_kernel_cornell_nq },
		  { (const void*)ssx_debug_step_kernel_plane, (const void*)ssx_debug_step_kernel_plane_nq } },
		{ { (const void*)ssx_debug_step_kernel_glibc, (const void*)ssx_debug_step_kernel_nq_glibc }, { (const void*)ssx_debug_step_kernel_cornell_glibc, (const void*)ssx_debug_step_kernel_cornell_nq_glibc },
		  { (const void*)ssx_debug_step_kernel_plane_glibc, (const void*)ssx_debug_step_kernel_plane_nq_glibc } } };
	const uint32_t* d_in = d_rows.as<uint32_t>();
	uint32_t* d_o = d_out.as<uint32_t>();
	void* args[] = { &a, &d_in, (void*)&n_tiles, &n_rounds, &d_o };
	SSX_HIP(ctx, hipLaunchKernel(kStepKernels[variant][ctx->topology][narrow], dim3((n_tiles + 3u) / 4u), dim3(256), args, path_lds_bytes(a.blob_words, qw), ctx->stream));
	SSX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	SSX_HIP(ctx, hipMemcpy(out, d_out.ptr, out_bytes, hipMemcpyDeviceToHost));
	return SSX_OK;
}

#ifdef SSX_LANESTAT // profiling build only (tools/lanestat.py)
int ssx_lanestat(unsigned long long* out, int reset) {
	if (reset) { unsigned long long z[2 * SSX_NSTAT] = {}; return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_lanestat), z, sizeof z); }
	(void)hipDeviceSynchronize();
	return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lanestat), 2 * SSX_NSTAT * sizeof(unsigned long long));
}
#endif
#ifdef SSX_REGTIME // profiling build only (tools/regtime.py)
int ssx_regtime(unsigned long long* out, int reset) { // SSX_NTIME shader-clock sums, one per region (ssx_lanestat.h SSX_TIME)
	if (reset) { unsigned long long z[SSX_NTIME] = {}; return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_regtime), z, sizeof z); }
	(void)hipDeviceSynchronize();
	return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_regtime), SSX_NTIME * sizeof(unsigned long long));
}
#endif

int ssx_set_jit(ssx_ctx* ctx, int mode) {
	if (!ctx || mode < SSX_JIT_OFF || mode > SSX_JIT_BACKGROUND) return SSX_ERR_ARG;
	ctx->jit_mode = mode;
	return SSX_OK;
}

int ssx_jit_status(ssx_ctx* ctx, int wait_ms, char* message, size_t message_size) {
	if (!ctx) return SSX_ERR_ARG;
	if (ctx->rendering.load()) return fail(ctx, SSX_ERR_STATE, "render in progress");
	if (ctx->jit_pending && wait_ms != 0) {
		if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, SSX_ERR_DEVICE, "hipSetDevice failed");
		if (!ctx->jit_requested) { ssx_jit::request(ctx->jit_vid, ctx->variant); ctx->jit_requested = true; }
		(void)ssx_jit::wait(ctx->jit_vid, wait_ms < 0 ? 600000 : wait_ms, ctx->variant);
		maybe_swap_jit(ctx, 0);
	}
	copy_text(ctx->jit_message, message, message_size);
	return ctx->jit_state;
}

void ssx_jit_counters(uint64_t* compiled, uint64_t* disk_hits) {
	ssx_jit::Shared& S = ssx_jit::shared();
	std::lock_guard<std::mutex> g(S.m);
	if (compiled) *compiled = S.compiled;
	if (disk_hits) *disk_hits = S.disk_hits;
}

int ssx_debug_pass1_source(const uint8_t* vid, uint32_t n_quads, const char* name, char* out, size_t out_size) {
	if (!vid || !name || n_quads == 0 || n_quads > 32u) return SSX_ERR_ARG;
	ssx_jit::VidTable t(n_quads);
	for (uint32_t q = 0; q < n_quads; ++q) for (int v = 0; v < 4; ++v) t[q][v] = vid[4 * q + v];
	const std::string text = ssx_jit::pass1_source(name, t);
	copy_text(text, out, out_size);
	return (int)text.size();
}

int ssx_calibration_info(ssx_ctx* ctx, float* frames_per_sample, float* rays_left_per_sample, int* camera_rays_pretraced) {
	if (!ctx) return SSX_ERR_ARG;
	if (!ctx->have_scene) return fail(ctx, SSX_ERR_STATE, "no scene uploaded");
	if (frames_per_sample) *frames_per_sample = ctx->calib_frames;
	if (rays_left_per_sample) *rays_left_per_sample = ctx->calib_left;
	if (camera_rays_pretraced) *camera_rays_pretraced = ctx->pre_hits ? 1 : 0;
	return SSX_OK;
}

int ssx_scratch_info(ssx_ctx* ctx, uint64_t* sample_bytes, uint64_t* log_bytes) {
	if (!ctx) return SSX_ERR_ARG;
	if (sample_bytes) *sample_bytes = (uint64_t)sample_slots(ctx) * bytes_per_sample(ctx) + (ctx->spectral_moments ? (uint64_t)ctx->d_spectral_moments.bytes : 0u);
	if (log_bytes) *log_bytes = (uint64_t)ctx->d_logs.bytes;
	return SSX_OK;
}

int ssx_sums_info(ssx_ctx* ctx, uint64_t* units_parked, uint64_t* units_chained) {
	if (!ctx) return SSX_ERR_ARG;
	uint32_t c[4] = { 0u, 0u, 0u, 0u };
	if (ctx->d_unit_counter.ptr) {
		SSX_HIP(ctx, hipSetDevice(ctx->device));
		const int rc = wait_device_pending(ctx);
		if (rc) return rc;
		SSX_HIP(ctx, hipMemcpy(c, ctx->d_unit_counter.ptr, sizeof c, hipMemcpyDeviceToHost));
	}
	if (units_parked) *units_parked = c[2];
	if (units_chained) *units_chained = c[3];
	return SSX_OK;
}

int ssx_units_info(ssx_ctx* ctx, uint64_t* units_enqueued) {
	if (!ctx) return SSX_ERR_ARG;
	if (units_enqueued) *units_enqueued = ctx->units_enqueued.load();
	return SSX_OK;
}

int ssx_generate_info(ssx_ctx* ctx, uint64_t* generate_launches, uint64_t* fused_launches) {
	if (!ctx) return SSX_ERR_ARG;
	if (generate_launches) *generate_launches = ctx->launches_generated.load();
	if (fused_launches) *fused_launches = ctx->launches_fused.load();
	return SSX_OK;
}

int ssx_kernel_variant(ssx_ctx* ctx) { return (ctx && ctx->have_scene) ? (int)ctx->topology : -1; }

const char* ssx_kernel_name(ssx_ctx* ctx) {
	if (!ctx || !ctx->have_scene) return nullptr;
	if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
	uint32_t qw = 0;
	if (pick_queue(ctx, ctx->path_blob_words, &qw, nullptr) != SSX_OK) return nullptr;
	const bool narrow = qw == SSX_QUEUE_WORDS_NARROW;
	// (the _plain twins go by the general kernels' names here: ssx_switches_info says which of the two runs)
	const uint32_t named = ctx->variant == ssx_jit::kVariantPlain ? (uint32_t)SSX_LIBM_BUILD : ctx->variant;
	return ctx->topology == 3u ? kJitKernelNames[narrow] : kPathKernels[named][ctx->topology][narrow].name;
}

int ssx_switches_info(ssx_ctx* ctx) { return (ctx && ctx->have_scene) ? (ctx->variant == ssx_jit::kVariantPlain ? 1 : 0) : -1; }
int ssx_scene_traits(const ssx_scene_desc* s) {
	if (!s || s->struct_size != sizeof(ssx_scene_desc) || (s->n_quads && (!s->quads || !s->materials)) || (s->n_lights && !s->lights)) return -1;
	return (int)scene_traits_of(s);
}
int ssx_render_traits(const ssx_render_params* p) {
	if (!p || p->struct_size != sizeof(ssx_render_params)) return -1;
	return (int)render_traits_of(p, false);
}

int ssx_plan_info(ssx_ctx* ctx, float* frames_per_sample, int* fold_in_path_kernel) {
	if (!ctx) return SSX_ERR_ARG;
	if (!ctx->have_scene) return fail(ctx, SSX_ERR_STATE, "no scene uploaded");
	if (frames_per_sample) *frames_per_sample = ctx->calib_frames;
	if (fold_in_path_kernel) *fold_in_path_kernel = ctx->fuse_resolve ? 1 : 0;
	return SSX_OK;
}

int ssx_kernel_info(ssx_ctx* ctx, int* vgprs, int* sgprs, int* lds_bytes, int* scratch_bytes, int* max_blocks_per_cu) {
	if (!ctx) return SSX_ERR_ARG;
	SSX_HIP(ctx, hipSetDevice(ctx->device));
	hipFuncAttributes at;
	uint32_t qw = 0; int nb = 0;
	int r = pick_queue(ctx, ctx->path_blob_words, &qw, &nb);
	if (r) return r;
	const KernelRef k = path_kernel_ref(ctx, qw == SSX_QUEUE_WORDS_NARROW);
	if (k.mod) {
		int v = 0;
		SSX_HIP(ctx, hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_NUM_REGS, k.mod)); at.numRegs = v;
		SSX_HIP(ctx, hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, k.mod)); at.sharedSizeBytes = (size_t)v;
		SSX_HIP(ctx, hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, k.mod)); at.localSizeBytes = (size_t)v;
	} else SSX_HIP(ctx, hipFuncGetAttributes(&at, k.host));
	if (vgprs) *vgprs = at.numRegs;
	if (sgprs) *sgprs = 0;
	if (lds_bytes) *lds_bytes = (int)at.sharedSizeBytes + (int)path_lds_bytes(ctx->path_blob_words, qw);
	if (scratch_bytes) *scratch_bytes = (int)at.localSizeBytes;
	if (max_blocks_per_cu) *max_blocks_per_cu = nb;
	return SSX_OK;
}

} // extern "C"

#include "ssx_progressive.hip"
#include "ssx_spectral.hip"
#include "ssx_denoise.hip"
#include "ssx_develop.hip"
#include "ssx_optics.hip"
#include "ssx_defocus.hip"
#include "ssx_sensor.hip"
#include "ssx_glare.hip"
#include "ssx_display.hip"
#include "ssx_demod.hip"
#include "ssx_spectral_stats.hip"
#include "ssx_spectral_noise.hip"
#include "ssx_spectral_compare.hip"
#include "ssx_delta_e.hip"
