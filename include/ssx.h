/* ssx.h -- C ABI of the MI355X spectral path-tracing core (libssx_hip.so).
 *
 * This is the drop-in boundary for ONE path of geometrian/simple-spectral: the body of
 * Renderer::_render_threadwork (reference src/renderer.cpp:309-395) -- the tile loop, the
 * per-pixel sample loop (_render_pixel, :278-308) and the radiance recursion (_render_sample,
 * :104-277) -- between "Options + Scene + Color tables exist" and "framebuffer(i,j) is filled".
 * The reference has no FFI layer (single executable); the entry points below are what a
 * maintainer would bind in its place (INTEGRATION.md shows the C++ stub).
 *
 * Conventions: plain C, no exceptions cross the boundary.  Every function returns 0 (SSX_OK) or a
 * negative code mirroring the reference's `throw int` values (-1 data/I-O, -2 argument, -3 unknown
 * scene/variant; reference src/main.cpp:78,100, src/renderer.cpp:37, src/spectrum.cpp:19,181,197,
 * 208, src/material.cpp:17) plus device failures.  The host owns every pointer it passes; the
 * library copies what it needs during the call and owns all device allocations.
 * There is NO CPU fallback: without a gfx950 device ssx_create fails with SSX_ERR_DEVICE.
 */
#ifndef SSX_H
#define SSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this interface: what ssx_abi_version() of a library built from this header returns.  A host compares the two at load
 * (the C++ host in simple_spectral_amd/host/renderer.cpp and the Python binding do) and refuses a mismatch.
 *   1  rounds 1-2
 *   2  ssx_quad.is_light became the bitfield `flags` (SSX_PRIM_LIGHT | SSX_PRIM_TRI: other nonzero values are refused now);
 *      ssx_render_params.reserved became no_flat_field_correction (a stale nonzero value changes the image); SSX_MAX_QUADS 32 -> 128,
 *      SSX_MAX_TEXTURES and the struct sizes grew; ssx_set_jit takes a mode (default: background compilation); ssx_jit_status,
 *      ssx_jit_counters, ssx_sums_info, ssx_rccl_groups_made, ssx_done_tiles and ssx_render_params.tile_major and tile_skew (the
 *      struct grew by 8 bytes) are new.  Added since without a change of existing entry points or structures (same version): ssx_units_info,
 *      ssx_rccl_probe (round 6); ssx_render_params.libm, appended (a caller with the struct_size before it gets SSX_LIBM_BUILD); the progressive
 *      rendering, spectral output, denoising, develop and demodulated-denoising entry points below; ssx_debug_tile_mask and SSX_DBG_TRACE_MASKED;
 *      ssx_debug_spectral_accumulate; SSX_DBG_TRACE_TOPO; ssx_debug_fold; ssx_debug_step; ssx_debug_generate and ssx_generate_info. */
#define SSX_ABI_VERSION 2

enum {
	SSX_OK = 0,
	SSX_ERR_DATA = -1,    /* bad table / texture data */
	SSX_ERR_ARG = -2,     /* bad argument */
	SSX_ERR_SCENE = -3,   /* unknown scene / unsupported variant */
	SSX_ERR_DEVICE = -10, /* HIP failure or no device */
	SSX_ERR_STATE = -11   /* call not valid in the current state */
};

/* Compile-time constants of the reference this core is built for (src/stdafx.hpp:44-93). */
#define SSX_MAX_DEPTH 10u          /* MAX_DEPTH */
#define SSX_TILE_SIZE 8u           /* TILE_SIZE */
#define SSX_SAMPLE_WAVELENGTHS 4u  /* SAMPLE_WAVELENGTHS */
#define SSX_MAX_TEXTURES 64u       /* texture descriptors (16 bytes each) staged per workgroup; the texels stay in HBM */
#define SSX_MAX_QUADS 128u         /* Scene::primitives: the per-quad records are staged in LDS (160 bytes each; with more than
                                      32 primitives the intersection works through them in groups of 32 and, where the
                                      48 KB of scene tables would overflow, keeps its permuted vertex table in HBM) */

/* _Spectrum (reference src/spectrum.hpp:12-31): n uniform samples over [low,high]. */
typedef struct ssx_spectrum {
	uint32_t offset;   /* first sample in ssx_scene_desc.samples */
	uint32_t n;        /* >= 2 */
	float low, high;
	float delta_recip; /* float(n-1)/(high-low), src/spectrum.cpp:22-25 */
} ssx_spectrum;

/* Vertex (src/geometry.hpp:13-22) */
typedef struct ssx_vertex { float pos[3]; float st[2]; } ssx_vertex;

/* One primitive of Scene::primitives (src/scene.hpp:39).  PrimQuad = tri0(v00,v10,v11) + tri1(v00,v11,v01)
 * (src/geometry.hpp:76-103); normals are the host-computed PrimTri normals (src/geometry.hpp:68).
 * With SSX_PRIM_TRI in `flags` the primitive is a PrimTri (src/geometry.hpp:55-74) of v00, v10, v11: v01 and
 * normal1 are ignored, intersection tests the one triangle (src/geometry.cpp:12-101), and as a light it is
 * sampled by PrimTri::get_rand_toward (src/geometry.cpp:103-116: no triangle pick, so one random number fewer
 * than a quad, and no halving of the pdf, :141-145). */
enum { SSX_PRIM_LIGHT = 1u,      /* material->is_emissive() at construction, src/geometry.cpp:7-9 */
       SSX_PRIM_TRI = 0x100u };  /* PrimBase::TYPE::TRI (src/geometry.hpp:28-32); otherwise QUAD */
typedef struct ssx_quad {
	ssx_vertex v00, v10, v11, v01;
	float normal0[3], normal1[3];
	uint32_t material;
	uint32_t flags;    /* SSX_PRIM_LIGHT | SSX_PRIM_TRI (the field was `is_light` = 0 / 1 before the triangle kind existed) */
} ssx_quad;

enum { SSX_MTL_LAMBERTIAN = 0, SSX_MTL_MIRROR = 1 };   /* src/material.hpp:144-176 */
enum { SSX_ALBEDO_CONSTANT = 0, SSX_ALBEDO_TEXTURE = 1 }; /* MaterialSimpleAlbedoBase::MODE */

typedef struct ssx_material {
	uint32_t kind;
	uint32_t albedo_mode;
	uint32_t albedo_spectrum;   /* index into spectra (CONSTANT) */
	uint32_t albedo_texture;    /* index into textures (TEXTURE) */
	uint32_t emission_spectrum; /* index into spectra */
} ssx_material;

/* sRGB_ReflectanceTexture (src/material.hpp:14-45): RGB8, rows top to bottom. */
typedef struct ssx_texture { uint32_t width, height; const uint8_t* rgb; } ssx_texture;

/* RENDER_MODE_SPECTRAL_ALGNUM (src/stdafx.hpp:63-73): how a texel's linear RGB becomes a
 * reflectance spectrum (Color::lrgb_to_specrefl, src/util/color.cpp:167-232). */
enum { SSX_UPLIFT_OURS = 1, SSX_UPLIFT_MENG = 2, SSX_UPLIFT_JH = 3 };
/* `uplift` value for the reference's other build mode, RENDER_MODE_RGB (src/stdafx.hpp:91-93): no
 * spectra at all -- the integrator carries linear RGB, texels are used as they are (src/material.cpp:
 * 61-63), no wavelength is drawn (src/renderer.cpp:134-143), pixels are the plain mean of the
 * samples (:300-304) and the image returned is linear RGB + alpha, not XYZ.  The scene then encodes
 * every "spectrum" as the 4-sample table {r,g,b,0} with low = 0, delta_recip = 1, and lambda_min = 0,
 * lambda_step = 1 (the three components ride in the first three hero slots). */
enum { SSX_MODE_RGB = 0 };

/* Meng et al. 2015 grid (RENDER_MODE_SPECTRAL_MENG): the tables the reference compiles in from
 * src/meng-et-al.-2015/spectra_xyz_5nm_380_780_0.97.h, here passed as data (this library ships no
 * copy of them; see simple_spectral_amd/meng.py for the file format and converter). */
typedef struct ssx_meng_grid {
	uint32_t grid_w, grid_h;       /* spectrum_grid_width/height (:2-3) */
	uint32_t n_points, n_samples;  /* data points; spectrum_num_samples (:9) */
	float sample_min, sample_max;  /* spectrum_sample_min/max (:6-7) */
	float xy_to_uv[6];             /* spectrum_mat_xy_to_uv (:23-27) */
	const int32_t* cells;          /* grid_w*grid_h x {inside, num_points, idx[6]} (spectrum_grid_cell_t, :58-63) */
	const float* points;           /* n_points x {xystar[2], uv[2], spectrum[n_samples]} (spectrum_data_point_t) */
} ssx_meng_grid;

/* Everything the kernel reads: the flattened Scene (src/scene.hpp:16-66) + Color::data tables
 * (src/util/color.hpp:22-68). */
typedef struct ssx_scene_desc {
	uint32_t struct_size; /* sizeof(ssx_scene_desc) */
	uint32_t reserved;
	double pv_inv[16];    /* camera.matr_PV_inv, column-major (src/scene.cpp:24) */
	float cam_pos[3];     /* camera.pos */
	float lambda_min;     /* LAMBDA_MIN */
	float lambda_step;    /* LAMBDA_STEP = (LAMBDA_MAX-LAMBDA_MIN)/4 (src/stdafx.hpp:289) */
	uint32_t spec_xbar, spec_ybar, spec_zbar;          /* std_obs_{x,y,z}bar */
	uint32_t spec_basis_r, spec_basis_g, spec_basis_b; /* basis_bt709.{r,g,b} */
	const ssx_spectrum* spectra;  uint32_t n_spectra;
	const float* samples;         uint32_t n_samples;
	const ssx_material* materials; uint32_t n_materials;
	const ssx_quad* quads;        uint32_t n_quads;   /* Scene::primitives, in order */
	const uint32_t* lights;       uint32_t n_lights;  /* Scene::lights (indices into quads) */
	const ssx_texture* textures;  uint32_t n_textures;
	/* srgb_to_lrgb(u8*(1/255)) for u8=0..255 (src/material.cpp:52-56, src/util/color.hpp:91-97):
	 * built by the host with the platform powf, exactly as the reference evaluates it per texel. */
	float srgb_to_linear[256];
	/* uplift variant; for SSX_UPLIFT_JH the Jakob-Hanika model (src/jakob-and-hanika-2019/
	 * rgb2spec.h:9-13): scale[jh_res], data[3*jh_res^3*3]; unused (0/NULL) for SSX_UPLIFT_OURS */
	uint32_t uplift;
	uint32_t jh_res;
	const float* jh_scale;
	const float* jh_data;
	/* SSX_UPLIFT_MENG: the grid (copied at upload); NULL otherwise.  Callers built against the
	 * struct without this field (smaller struct_size) keep working. */
	const ssx_meng_grid* meng;
	/* camera.dir (src/scene.hpp:21), read only by renders with ssx_render_params.no_flat_field_correction.
	 * Callers built against the struct without this field keep working (such renders are then refused). */
	float cam_dir[3];
	uint32_t reserved2;
} ssx_scene_desc;

/* One render = Renderer::render_start..render_wait (src/renderer.cpp:396-430) for this device's
 * share of the 8x8 tile list (src/renderer.cpp:396-409; row-major tile index t = ty*ceil(W/8)+tx). */
typedef struct ssx_render_params {
	uint32_t struct_size;
	uint32_t width, height;   /* Options::res */
	uint32_t spp;             /* Options::spp: the pixel mean divides by this */
	uint32_t indirect_only;   /* Options::indirect_only */
	uint32_t tile_first;      /* this device renders tiles t with t % tile_stride == tile_first ... */
	uint32_t tile_stride;     /* ... (1 = whole image); other pixels are written as 0 */
	uint32_t spp_per_launch;  /* progress/cancel granularity; 0 = library default */
	uint32_t no_explicit_light_sampling; /* 0 = EXPLICIT_LIGHT_SAMPLING defined (src/stdafx.hpp:44, the
	                             reference's default); 1 = the integrator it compiles without it */
	uint32_t no_flat_field_correction;   /* 0 = FLAT_FIELD_CORRECTION defined (src/stdafx.hpp:55, the reference's default:
	                             flux = radiance); 1 = the build without it: flux = radiance * dot(camera_ray_dir,
	                             camera.dir) (src/renderer.cpp:262-266).  (Was `reserved`, 0.) */
	uint32_t tile_major;      /* How ssx_render_start walks through the work, i.e. what a stopped render holds (the image of a finished render
	                             does not depend on it).  0: all owned tiles together, a range of samples per launch; after ssx_render_stop
	                             every pixel holds the mean over the samples done so far (ssx_done_spp).  1: the reference's way
	                             (src/renderer.cpp:340-409: the tile list from tile (0,0) upwards, every tile rendered to the full sample
	                             count): a range of tiles per launch; after ssx_render_stop the finished tiles hold their final value and the
	                             others are returned as zeros -- ssx_done_tiles says how many of the device's tiles, in ascending tile order,
	                             are finished, so that the host leaves its checkerboard where the reference does (src/renderer.cpp:388-394,
	                             src/framebuffer.cpp:15-32).  Ignored by ssx_render_device (which cannot be stopped). */
	uint32_t tile_skew;       /* The list the devices share out (tile_first / tile_stride) is the row-major tile list with tile row ty rotated by
	                             ty * tile_skew columns; 0 = the plain list.  With N devices and a tile row of a multiple of N tiles the plain list
	                             gives every device vertical stripes of the image, whose cost differs (Cornell box at N = 8: the outer stripes are
	                             7 % cheaper than the inner ones); tile_skew = 1 gives diagonals.  All devices of a render use the same value;
	                             the image does not depend on it.  Any value is accepted and taken modulo the number of tile columns (the
	                             rotation (ty * tile_skew) % tiles_x is what enters: kernels, C++ host and Python mask agree for every value). */
	uint64_t seed;            /* seeding contract below */
	uint32_t libm;            /* Which sinf / cosf / acosf the integrator evaluates (the reference calls the platform's, src/util/random.cpp,
	                             src/util/spherical-tri.cpp).  SSX_LIBM_BUILD (0, default): the functions include/ssx_fmath.h defines, the same
	                             on every platform.  SSX_LIBM_GLIBC_2_35: glibc 2.35's x86-64 functions (FMA variant), restated by
	                             include/ssx_glibc_math.h -- the image of the reference built and run on a stock x86-64 glibc 2.35 system.  The
	                             kernels are the *_glibc twins of the default ones.  Other values: SSX_ERR_ARG.  (Appended: a caller that passes
	                             struct_size = offsetof(ssx_render_params, libm) gets SSX_LIBM_BUILD.) */
	uint32_t reserved3;       /* padding (the struct's size is a multiple of 8); ignored */
} ssx_render_params;
enum { SSX_LIBM_BUILD = 0, SSX_LIBM_GLIBC_2_35 = 1 };

/* Seeding contract (build-defined; the shipped reference is racy):
 * sample k of pixel p=j*W+i uses its own PCG32 stream
 *     a = mix64(seed + G*(p+1)); b = mix64(a + G*(k+1)); state = b; inc = mix64(b ^ C) | 1
 * with G=0x9E3779B97F4A7C15, C=0xDA3E39CB94B95BDB and mix64 the splitmix64 finaliser; samples of
 * a pixel are accumulated in ascending k as double += float(sample*0.001f) (src/renderer.cpp:
 * 292-296).  The image is therefore independent of tile partition, launch size and device. */

typedef struct ssx_ctx ssx_ctx;

/* Renderer::Renderer / ~Renderer (src/renderer.cpp:12-51).  device = HIP ordinal. */
int ssx_create(int device, ssx_ctx** out);
void ssx_destroy(ssx_ctx* ctx);

/* Replaces handing `Scene*` + `Color::data` to the worker threads (src/renderer.cpp:33,163,189). */
int ssx_upload_scene(ssx_ctx* ctx, const ssx_scene_desc* scene);

/* Renderer::render_start (src/renderer.cpp:396-422): returns at once, work proceeds on the device. */
int ssx_render_start(ssx_ctx* ctx, const ssx_render_params* params);
/* Renderer::render_stop (src/renderer.hpp:77): cooperative, takes effect between launches. */
int ssx_render_stop(ssx_ctx* ctx);
/* Renderer::is_rendering (src/renderer.hpp:81) */
int ssx_is_rendering(ssx_ctx* ctx);
/* the `part` of Renderer::_print_progress (src/renderer.cpp:75): fraction in [0,1] */
float ssx_progress(ssx_ctx* ctx);
/* Samples per pixel accumulated so far by the render started last (== ssx_render_params.spp once it has completed).  After
 * ssx_render_stop the image is the mean over THESE samples for every pixel -- the reference instead keeps finished tiles at
 * full spp next to untouched checkerboard tiles (src/renderer.cpp:388-394, src/framebuffer.cpp:9-33); with several devices
 * each context may have stopped at another count, which the caller can read here. */
uint32_t ssx_done_spp(ssx_ctx* ctx);
/* tile_major renders: the device's tiles (those with t % tile_stride == tile_first, in ascending order) finished so far; after a
 * completed render: all of them.  Other renders: 0 while rendering, all of them when done. */
uint32_t ssx_done_tiles(ssx_ctx* ctx);
/* Renderer::render_wait (src/renderer.cpp:423-430) + read-back of what `framebuffer(i,j)=...`
 * (src/renderer.cpp:298) would receive BEFORE ciexyz_to_srgb: float4 {X,Y,Z,alpha} per pixel,
 * index j*W+i, row 0 = bottom (src/framebuffer.hpp:26-34).  xyza_out may be NULL. */
int ssx_render_wait(ssx_ctx* ctx, float* xyza_out);

/* Same render, enqueued on the caller's HIP stream into a caller-owned DEVICE buffer of
 * width*height float4 (no host synchronisation; used when the framebuffer stays on the GPU, e.g.
 * for the RCCL reduce).  hip_stream is a hipStream_t (NULL = default stream). */
int ssx_render_device(ssx_ctx* ctx, const ssx_render_params* params, void* d_xyza_out, void* hip_stream);
/* ssx_render_device only enqueues -- fills and kernels on hip_stream, no allocation and no synchronisation once the context's
 * buffers have the size the render needs -- so it may be called on a stream that is being captured into a hipGraph (launch-bound
 * small renders).  Then: run the same render once outside the capture first (sizes the buffers), let earlier renders of the context
 * finish before the capture (ssx_render_device_wait), do not time it (ssx_set_timing), and order the graph's replays against every
 * other use of the context yourself; otherwise SSX_ERR_STATE. */
/* Waits on the host for the work ssx_render_device has queued for this context (the caller's streams are not touched otherwise). */
int ssx_render_device_wait(ssx_ctx* ctx);

/* ssx_render_start's result stays in a context-owned DEVICE buffer; these give the C++ host's multi-GPU
 * combine access to it (north_star: "final reduce over xGMI of the per-GPU framebuffer"; the reference
 * has one address space and no such step).  ssx_render_wait(ctx, NULL) skips the copy to the host. */
void* ssx_device_framebuffer(ssx_ctx* ctx);            /* float4[width*height] on ctx's device, valid until the next render */
int ssx_device_index(ssx_ctx* ctx);
int ssx_read_framebuffer(ssx_ctx* ctx, float* xyza_out); /* device framebuffer -> host */
/* d_dst (on ctx's device) += d_src (on HIP device src_device), both float4[width*height]: one
 * hipMemcpyPeerAsync (device to device over xGMI) into a staging buffer + one add kernel.  Every pixel
 * is nonzero on exactly one device (tile_first/tile_stride), so the sum is exact.  Synchronous. */
int ssx_accumulate_peer(ssx_ctx* ctx, void* d_dst, int src_device, const void* d_src, uint32_t width, uint32_t height, void* hip_stream);

/* The same combine as one RCCL reduce (sum, float) of the n contexts' device framebuffers into ctxs[0]'s: one rank per
 * context of this process (ncclCommInitAll), the contexts on n different devices.  RCCL is loaded on first use; the
 * communicators are created by the first combine of a group of contexts and kept in them for the next (a call with other
 * contexts, or the same in another order, replaces them; ssx_destroy releases a context's). */
int ssx_reduce_rccl(ssx_ctx** ctxs, int n, uint32_t width, uint32_t height);
/* A dry run of that combine on whatever devices this process sees, REPORTING what it finds instead of failing on it: device list with
 * free memory, peer access pair by pair, ncclCommInitAll over all of them, one grouped 4 MiB ncclReduce to device 0 checked element by
 * element.  `report` receives JSON text.  Returns the number of devices the reduce went through correctly (0: it did not happen -- the
 * report says why), or SSX_ERR_ARG.  Needs no context; releases what it created.  (bench.py --dist-dry-run prints it next to the
 * per-rank view of torch.distributed.) */
int ssx_rccl_probe(char* report, size_t report_size);
/* Groups of communicators ssx_reduce_rccl has created in this process so far (a repeated combine must not add any). */
uint64_t ssx_rccl_groups_made(void);

/* Last error text for ctx (or for ssx_create when ctx is NULL). */
const char* ssx_last_error(const ssx_ctx* ctx);

/* Measurement aid: when enabled, HIP events are recorded on the launch stream around the stages
 * of every launch; ssx_get_timing waits for them and returns (and clears) the summed milliseconds
 * {generate (camera rays + their hits), path megakernel, resolve, accumulate} since the last call.  (The resolve
 * stage -- fold of the recursion + XYZ -- runs inside the path kernel: its slot reads ~0.) */
int ssx_set_timing(ssx_ctx* ctx, int enable);
int ssx_get_timing(ssx_ctx* ctx, float stage_ms[4]);

/* Introspection: ABI version, and per-kernel resource usage for reports. */
int ssx_abi_version(void);
int ssx_kernel_info(ssx_ctx* ctx, int* vgprs, int* sgprs, int* lds_bytes, int* scratch_bytes, int* max_blocks_per_cu);
/* What ssx_upload_scene's calibration render (64x64x4 samples of the scene, fixed seed) found: frames
 * (continued interactions) per sample.  fold_in_path_kernel is always 1: the fold of the recursion runs at
 * the end of each wave's work unit inside the path kernel (the stand-alone fold kernel of earlier versions
 * is gone: the levels live in per-wave logs that are recycled while the kernel runs). */
int ssx_plan_info(ssx_ctx* ctx, float* frames_per_sample, int* fold_in_path_kernel);
/* More of what the calibration render found, and the choice made from it: rays per sample that left the scene (camera and
 * continuation rays), and whether the camera rays are traced ahead of the path loop by the generate kernel (1: where at
 * least ~0.3 rays per sample leave the scene, e.g. the open Cornell box) or inside it like every other ray (0).  A
 * performance choice only: same bits.  The environment variable SSX_PRE_HITS=0/1 at upload overrides it. */
int ssx_calibration_info(ssx_ctx* ctx, float* frames_per_sample, float* rays_left_per_sample, int* camera_rays_pretraced);
/* Device scratch the context holds right now: the per-sample arrays of the largest launch so far (48 bytes per sample in
 * flight: camera ray / result, stream / tail word, camera hit; 64 while spectral output is on: + hero flux; while the spectral moments are on, the second moments Q are counted
 * with them: owned tiles x bins x 64 x 8 bytes) and the persistent waves' level logs (a fixed size per
 * device and unit size: wave slots x 2 units x cohorts x 128 records x 582 bytes). */
int ssx_scratch_info(ssx_ctx* ctx, uint64_t* sample_bytes, uint64_t* log_bytes);
/* How the ordered binary64 pixel sums (src/renderer.cpp:292-295: a pixel's samples are added in ascending k) went, counted since
 * ssx_create: work units of the path kernel (8x8 tile x 4 or 8 consecutive samples) that finished before their tile's turn had
 * reached them and parked their samples instead of waiting, and how many of those were then added by the wave in front of them
 * (the rest had been given the turn before their mark was in place, and added themselves).  No wave ever waits for another; a
 * large count is normal for a device that owns few tiles at many samples per pixel (a rank of a multi-GPU render: three quarters
 * of the units at 512 tiles x 2048 samples).  Waits for a queued ssx_render_device. */
int ssx_sums_info(ssx_ctx* ctx, uint64_t* units_parked, uint64_t* units_chained);
/* Work units the context has enqueued since ssx_create (every launch of the path kernel: tiles owned x groups of consecutive samples;
 * the calibration render of ssx_upload_scene not counted): the denominator of the counts above, from the code that sizes the
 * launches -- a host need not re-derive the unit size (bench.py did, and was wrong for a render split into batches). */
int ssx_units_info(ssx_ctx* ctx, uint64_t* units_enqueued);
/* ... and how those launches got their samples, counted the same way: launches in front of which ssx_generate_kernel ran, and launches whose path kernel
 * made its samples itself in its refill (kernels of the plane topology with camera rays traced in the path loop; SSX_FUSE_GEN=0 under SSX_DEBUG_ENV=1
 * keeps the generate kernel).  From the code that decides it, per launch.  Either may be NULL. */
int ssx_generate_info(ssx_ctx* ctx, uint64_t* generate_launches, uint64_t* fused_launches);
/* Which path kernel the uploaded scene runs: 0 = the generic one (pass 1 of the intersection loops over the
 * quads), 1 / 2 = the kernel whose pass 1 is specialised to the mesh topology of the reference's Cornell box /
 * plane scene (the scene's quad corners coincide in exactly that pattern; positions are free), 3 = specialised to
 * the scene's own topology at run time (ssx_set_jit).  A performance
 * choice only: same bits.  The environment variable SSX_GENERIC_KERNEL forces 0 at upload.  -1: no scene. */
int ssx_kernel_variant(ssx_ctx* ctx);
/* Pass 1 of the intersection is straight-line code for the two mesh topologies of the reference's built-in scenes; a scene whose
 * corners coincide in another pattern starts on a generic loop (~25 % slower).  Such a scene (at most 32 primitives, all quads) gets
 * kernels compiled for ITS pattern with hipRTC (a second or two per pattern), kept in this process's memory and in a disk cache
 * ($SSX_CACHE_DIR, else $XDG_CACHE_HOME/ssx, else ~/.cache/ssx: a later process starts specialised at once, < 50 ms).  When:
 *   SSX_JIT_BACKGROUND (default)  ssx_upload_scene never waits: code already in memory or on disk is used at once, else the generic
 *                                 kernel serves the scene and a background thread compiles once the context has rendered 32 M samples on
 *                                 it; the context switches kernels at the start of a later render (ssx_render_device / ssx_render_start,
 *                                 and between the launches of an asynchronous render).
 *   SSX_JIT_AT_UPLOAD             ssx_upload_scene compiles on the calling thread when nobody has the code yet.
 *   SSX_JIT_OFF                   generic kernel.
 * Same bits in every case.  A failure of any kind -- no libhiprtc, no HIP headers ($SSX_ROCM_INCLUDE, $ROCM_PATH/include,
 * /opt/rocm/include), a compile error, an unwritable cache -- leaves the scene on the generic kernel; ssx_jit_status tells.
 * libm (ssx_render_params.libm): the two modes' kernels of a pattern are separate code objects (and cache files).  SSX_JIT_AT_UPLOAD compiles
 * the default mode's; SSX_JIT_BACKGROUND asks for those of the libm the context renders in at the time.  Once the context runs its own
 * kernels, the first render in the other libm compiles that mode's on the calling thread (or takes them from memory / the disk cache);
 * should that fail, the render fails (SSX_ERR_STATE: the generic kernels cannot read the specialised scene tables). */
enum { SSX_JIT_OFF = 0, SSX_JIT_AT_UPLOAD = 1, SSX_JIT_BACKGROUND = 2 };
int ssx_set_jit(ssx_ctx* ctx, int mode);
/* Where the uploaded scene's own kernels stand.  wait_ms != 0 first asks for the compilation if nobody has (whatever the context has
 * rendered so far), waits up to wait_ms milliseconds (< 0: until done) for it, and switches kernels if it has arrived.  message
 * (optional) receives why a compilation failed.  Not while an asynchronous render runs. */
enum { SSX_JIT_STATE_NONE = 0,              /* nothing to specialise: a built-in topology, triangles or > 32 primitives, or SSX_JIT_OFF */
       SSX_JIT_STATE_GENERIC_MEANWHILE = 1, /* the generic kernel serves; the scene's own code is not there (yet) */
       SSX_JIT_STATE_SPECIALISED = 2,       /* the scene's own kernels run (ssx_kernel_variant() == 3) */
       SSX_JIT_STATE_FAILED = -1 };         /* the generic kernel serves for good; see message */
int ssx_jit_status(ssx_ctx* ctx, int wait_ms, char* message, size_t message_size);
/* Patterns compiled by this process so far, and patterns it took from the disk cache (tests, start-up reports). */
void ssx_jit_counters(uint64_t* compiled, uint64_t* disk_hits);
/* The name of the path kernel the context launches for the uploaded scene, as a profiler lists it
 * ("ssx_render_kernel", "..._cornell", "..._plane", each also with "_nq": the variants with narrow shadow-ray
 * queue entries, taken where they let one more workgroup live on a CU; after a render with libm = SSX_LIBM_GLIBC_2_35
 * the same names with "_glibc" appended, after one with spectral output on with "_flux" -- the run-time compiled "ssx_render_kernel_jit" keeps
 * its name).  NULL: no scene. */
const char* ssx_kernel_name(ssx_ctx* ctx);
/* Render switches compiled into the path kernel.  The reference fixes its switches when it is built (src/stdafx.hpp); here each is a run-time
 * variant.  A render and a scene that are the reference's default build on Lambertian surfaces and quad lights -- none of the traits below -- run
 * the "_plain" twin of the kernel ssx_kernel_name names (same bits: the tests on the switches are compiled out of its loop, nothing else changes;
 * ssx_kernel_name keeps reporting the name without the suffix).  Any trait sends the render to the general kernel.
 * ssx_scene_traits / ssx_render_traits: the traits of a scene description / of render parameters, 0 = plain; host arithmetic only, no device and no
 * context (-1: bad argument).  ssx_switches_info: 1 = the context's current (or last) render ran, or a render with default parameters would run,
 * the kernel with the switches compiled in; 0 = the general kernel; -1 = no scene.  ssx_debug_samples always runs the general kernel (its
 * renders keep every sample).  SSX_PLAIN_KERNEL=0 under SSX_DEBUG_ENV=1 forces the general kernels (A/B runs, tests). */
enum { SSX_TRAIT_INDIRECT_ONLY = 1u, SSX_TRAIT_NO_ELS = 2u, SSX_TRAIT_MIRROR = 4u, SSX_TRAIT_TRI_LIGHT = 8u, SSX_TRAIT_UPLIFT = 16u,
       SSX_TRAIT_RGB_MODE = 32u, SSX_TRAIT_NO_FLAT_FIELD = 64u, SSX_TRAIT_KEEP_SAMPLES = 128u,
       SSX_TRAIT_LIBM = 256u, SSX_TRAIT_SPECTRAL_BINS = 512u, SSX_TRAIT_FORCED_OFF = 1024u }; /* (the last three: kernels that keep the general body, and the switch) */
int ssx_scene_traits(const ssx_scene_desc* scene);
int ssx_render_traits(const ssx_render_params* params);
int ssx_switches_info(ssx_ctx* ctx);

/* ---- Progressive rendering: continue, checkpoint / resume, noise estimate (appended; same ABI version) --------------------------------
 * A pixel's sum is double += float(sample * 0.001f) in ascending k and is scaled by 1000 / spp only when the image is made (seeding
 * contract above), so samples [0,a) followed by [a,b) leave the same bits as [0,b): a render can be taken up again where it ended.
 * The context keeps a CONTINUABLE state -- the render parameters, ssx_done_spp and valid sums.  It is set by an ssx_render_start that walked
 * through the samples (tile_major = 0) and finished or was stopped, by a tile_major one that FINISHED, and by ssx_sums_import; it is cleared
 * by ssx_upload_scene, ssx_render_device, ssx_debug_samples, a failed render and a stopped tile_major render. */

/* Samples [done, done + spp_more) of every owned pixel with the stored parameters, onto the existing sums; asynchronous like
 * ssx_render_start (stop / wait / is_rendering as there; ssx_progress is this call's fraction, ssx_done_spp counts from zero over the whole
 * history).  The image is then the mean over done + spp_more samples (or over the count reached when stopped).  The launch size is chosen
 * as ssx_render_start chooses it, from spp_more.  SSX_ERR_STATE: nothing to continue, or a render is running; SSX_ERR_ARG: spp_more == 0, or
 * more than 2^32 - 1 samples in all. */
int ssx_render_continue(ssx_ctx* ctx, uint32_t spp_more);

/* What a set of exported sums belongs to. */
typedef struct ssx_sums_info_t {
	uint32_t struct_size;     /* sizeof(ssx_sums_info_t) */
	uint32_t width, height;
	uint32_t done_spp;        /* samples per pixel the sums hold */
	uint64_t seed;
	uint32_t indirect_only, no_explicit_light_sampling, no_flat_field_correction, libm; /* as in ssx_render_params */
	uint32_t rgb_mode;        /* scene uploaded with uplift == SSX_MODE_RGB */
	uint32_t tile_first, tile_stride, tile_skew; /* whose tiles the exporter owned (every other pixel is +0) */
	uint32_t noise_batches;   /* B of the noise estimate below; 0: none */
	uint32_t reserved;
	uint64_t scene_digest;    /* ssx_scene_digest of the exporter's scene */
} ssx_sums_info_t;
/* A 64-bit digest of the uploaded scene: its packed tables (without device addresses), the uplift's table and the texels.  The same
 * description gives the same value in every process and on every device.  0: no scene. */
uint64_t ssx_scene_digest(ssx_ctx* ctx);
/* The raw binary64 accumulators, row-major [height][width][4] (row 0 = bottom), +0 for pixels the context does not own; noise_s2
 * ([height][width] or NULL) receives S2 of the noise estimate (zeros when there is none: info->noise_batches == 0).  One kernel turns the
 * device's [tile][component][pixel] layout into this one; the host gets one contiguous copy.  Needs the continuable state. */
int ssx_sums_export(ssx_ctx* ctx, ssx_sums_info_t* info, double* sums, double* noise_s2);
/* The inverse: the context takes, from the whole array, the tiles it owns under `params` (tile_first / tile_stride / tile_skew may differ
 * from the exporter's; params->spp is ignored), becomes continuable at info->done_spp and makes the image, so that ssx_read_framebuffer
 * returns the checkpointed one.  SSX_ERR_ARG when size, seed, a flag (indirect_only, no_explicit_light_sampling, no_flat_field_correction,
 * libm, rgb_mode) or scene_digest differ from params and the uploaded scene, or when the context would own a tile the exporter did not
 * (info->tile_first / tile_stride / tile_skew: one rank's unmerged export holds +0 there): ssx_last_error names the field.  With the noise estimate on,
 * noise_s2 and info->noise_batches carry it on; without them the imported sum counts as one batch. */
int ssx_sums_import(ssx_ctx* ctx, const ssx_render_params* params, const ssx_sums_info_t* info, const double* sums, const double* noise_s2);

/* Noise estimate by batch means (default off: nothing runs and nothing is allocated).  When on, the sample-walking render loop (start and
 * continue) runs one small kernel after each launch range [k0,k1): per owned pixel, on component 1 of the sums (Y; G in RGB mode), in
 * binary64 without contraction
 *     d = A_now - A_prev;   S2 += d*d / (double)(k1-k0);   A_prev = A_now
 * -- 16 bytes of state per pixel and a batch count B on the host.  ssx_render_start resets the state, ssx_render_continue and
 * ssx_sums_import carry it on (after an import A_prev is the imported sum).  With N = ssx_done_spp and A the current sum, the variance of the
 * pixel's MEAN is
 *     v = ((S2 - A*A/N) / (B-1)) / N
 * the between-batch estimator, exact in expectation also for batches of unequal size; undefined for B < 2.  The device evaluates it with
 * + - * / only and clamps at 0 by a compare, so it is reproducible bit for bit; square roots and ratios are the host's.
 * (Switching it on while continuable sums exist counts those as one batch; so do the sums of a finished tile_major render, which takes no
 * batches itself.)  Not while a render runs. */
int ssx_set_noise_estimate(ssx_ctx* ctx, int enable);
/* v per pixel (v_out: [height][width] or NULL; 0 for pixels the context does not own) and summary = { sum of v, sum of A/N, owned pixels, B }
 * over the owned pixels, added on the host one after the other in row-major order -- the ranks of a multi-GPU render are combined by adding
 * their summaries.  The image-level figure is defined as
 *     noise = sqrt(summary[0] / n) / (summary[1] / n),   n = summary[2]
 * the RMS standard error of the pixel means relative to the mean luminance (both in units of sample * 0.001: the constant 1000 of the image
 * cancels).  SSX_ERR_STATE: the estimate is off, or B < 2. */
int ssx_noise_info(ssx_ctx* ctx, double* v_out, double summary[4]);

/* ---- Spectral radiance output: per-pixel wavelength bins (appended; same ABI version) ------------------------------------------------
 * The integrator carries four hero wavelengths per sample, lambda_0 + i * lambda_step (i = 0..3; lambda_0 drawn in [lambda_min, lambda_min +
 * lambda_step]), and projects their fluxes onto the observer at once (flux_to_xyz).  With spectral output on, the fluxes are also binned by wavelength.
 * The definition is this library's (the reference has no such output):
 *   B bins, B in {4, 8, ..., 64} (a multiple of 4), M = B / 4.  Bin b covers [lambda_min + b*w, lambda_min + (b+1)*w) with w = lambda_step / M, so
 *   component i of a sample always falls into bin i*M + m, with one m per sample.  For sample k of pixel p, with f[0..3] the hero flux handed to
 *   flux_to_xyz (i.e. after the no_flat_field_correction multiply):
 *       t = (lambda_0 - lambda_min) / lambda_step          binary32, IEEE division, no contraction
 *       m = min(M-1, (uint32)(t * (float)M))               binary32 multiply, truncation
 *       S[p][i*M + m] += (double)f[i]   (i = 0..3);   N[p][m] += 1
 *   in ascending k, like the pixel sums (binary64 addition is not associative): the result does not depend on tile partition, launch size or device
 *   count.  mean[p][b] = N[p][b % M] ? (float)(S[p][b] / (double)N[p][b % M]) : 0.0f.  A sample that hit nothing contributes f = 0 and counts; a
 *   non-finite flux is added as it is; pixels a context does not own read as 0.
 * The state is valid from zero samples or not at all: an ssx_render_start that walks through the samples (tile_major = 0) resets it and accumulates,
 * ssx_render_continue carries it on; whatever invalidates the pixel sums (ssx_upload_scene, ssx_debug_samples, a failed render) and a changed bin
 * count clear it; ssx_sums_import ALONE leaves it invalid (pixel sums carry no bins: a continue after an import renders normally, and
 * ssx_spectral_read returns SSX_ERR_STATE) -- ssx_spectral_import, called on top of it with the bins of the same samples, makes it valid again, so that a
 * checkpoint which carries the bins (libssx_host.so: "SSXCKPT2") resumes with them.  The XYZ image of a render does not depend on whether spectral output is on.
 * While it is on, refused with SSX_ERR_ARG: renders of a scene in SSX_MODE_RGB, libm = SSX_LIBM_GLIBC_2_35, tile_major renders and
 * ssx_render_device.  These are out of scope so far, not limits of the design (the flux-storing kernels exist for the default libm only, and only
 * the sample walk runs the binning kernel between its launches). */

/* bins: 0 = off (default: nothing allocated, nothing launched, the default kernels), else B.  While on, the path kernels are the "_flux" twins of the
 * default ones, which also store every sample's hero flux (16 more bytes per sample in flight: ssx_scratch_info), and the sample walk runs one small
 * kernel per launch that bins them.  Not while a render runs (SSX_ERR_STATE); other values of bins: SSX_ERR_ARG. */
int ssx_set_spectral_bins(ssx_ctx* ctx, uint32_t bins);
typedef struct ssx_spectral_info_t {
	uint32_t struct_size;     /* sizeof(ssx_spectral_info_t) */
	uint32_t width, height;
	uint32_t bins;            /* B */
	uint32_t done_spp;        /* samples per pixel the bins hold (== ssx_done_spp) */
	uint32_t reserved;
	float lambda_min;         /* lower edge of bin 0 */
	float bin_width;          /* w = lambda_step / M (binary32); bin b's centre is lambda_min + (b + 0.5) * w */
} ssx_spectral_info_t;
/* Row-major (row 0 = bottom) mean [height][width][B] (float), sums [height][width][B] (the binary64 accumulators S) and counts [height][width][M];
 * any of the three may be NULL.  info is filled.  SSX_ERR_STATE: spectral output is off, a render runs, or the context holds no valid bins. */
int ssx_spectral_read(ssx_ctx* ctx, ssx_spectral_info_t* info, float* mean, double* sums, uint32_t* counts);
/* The inverse of ssx_spectral_read(sums, counts), for a checkpoint: the context takes, from the whole-image arrays sums [height][width][B] and counts
 * [height][width][M] (row-major, row 0 = bottom), the tiles it owns under its current parameters -- whoever exported them may have owned other tiles, as long
 * as the arrays hold every pixel this context owns: one rank's unmerged export holds zeros elsewhere (merge the ranks' exports by ownership first).  One
 * kernel, a transposition through LDS per owned 8x8 tile; tile lanes outside a ragged image receive +0 / 0, as a fresh render leaves them.
 * Valid only DIRECTLY ON TOP OF ssx_sums_import: the context is continuable, its pixel sums came from that call and nothing has rendered onto them since
 * (ssx_sums_import alone behaves as before: the bins invalid).  On success the context is exactly what it would be had it rendered the ssx_done_spp samples
 * itself: ssx_render_continue carries the bins on, ssx_spectral_read, ssx_denoise_spectral, ssx_spectral_develop and the _demod entry points work from them.
 * The same kernel checks what it takes: every sample is counted exactly once, so over an owned in-image pixel's M counts the sum is done_spp.
 * SSX_ERR_STATE: spectral output is off, a render runs, or there is no such import underneath.  SSX_ERR_ARG, ssx_last_error naming the field: width or height
 * differ from the context's; info->bins from its bin count; info->done_spp from ssx_done_spp; lambda_min or bin_width, compared as bits, from the uploaded
 * scene's; the check of the counts fails; what a render with spectral output is refused for (SSX_MODE_RGB, libm).  After a refusal the bins are invalid and the
 * pixel sums of ssx_sums_import are what they were: a continue renders normally.  done_spp == 0 is legal (all arrays zero). */
int ssx_spectral_import(ssx_ctx* ctx, const ssx_spectral_info_t* info, const double* sums /* [H][W][B] */, const uint32_t* counts /* [H][W][M] */);

/* ---- Denoising: first-hit guide buffers and a variance-guided a-trous filter (appended; same ABI version) -----------------------------------
 * The definitions are this library's (the reference has nothing like them).  Unless said otherwise everything is binary32 with IEEE + - * / and sqrtf,
 * no contraction, no transcendental, operations in the order written: a restatement in numpy gives the same bits (tests/denoise_ref.py).
 *
 * GUIDE BUFFERS, for every pixel (i, j) of a width x height image; they do not depend on ownership, seed or spp.  One camera ray through the pixel
 * centre -- camera_dir at ((double)i + 0.5, (double)j + 0.5), normalised and rounded to float exactly as a sample's ray is, no random number -- is
 * traced by the device function behind SSX_DBG_TRACE with no quad ignored:
 *     prim    uint32: the primitive's index, 0xFFFFFFFF for a miss
 *     depth   the hit distance, 0.0f for a miss
 *     normal  [3]: the hit triangle's stored normal (ssx_quad.normal0 / normal1), zeros for a miss
 *     albedo  [4]: what the device function behind SSX_DBG_ALBEDO returns for (prim, st of the hit, lambda_g), zeros for a miss; emission is no part of it.
 *             lambda_g = lambda_min + 0.5f * lambda_step; in SSX_MODE_RGB lambda_g = 0 (the components are then r, g, b, 0)
 *
 * VARIANCE IN IMAGE UNITS.  var[p] = (float)(v[p] * (s * s)), the product in binary64, with v what ssx_noise_info returns per pixel and s the factor the
 * image applies to the mean of the sums: 1000, or 1 in SSX_MODE_RGB.
 *
 * FILTER.  Parameters: levels L in 1..6, sigma_l > 0, sigma_a > 0.  Inputs per pixel: c = (X, Y, Z, A), var (>= 0 where finite), prim, albedo[4].
 * valid(p): X, Y, Z and var are all finite.  h = {1/16, 1/4, 3/8, 1/4, 1/16}; inv_sa2 = 1.0f / (sigma_a * sigma_a).  Levels l = 0 .. L-1 with step
 * st = 2^l, each reading the previous level's c and var.  An invalid p keeps its c and var at every level.  For a valid p:
 *     g   = sum k3*var[q] / sum k3 over the 3x3 neighbours q at distance 1 (not st) that are inside the image and valid, k3 = {1,2,1} x {1,2,1},
 *           both sums accumulated row-major (dy outer, dx inner, ascending), centre included
 *     den = sigma_l * sqrtf(g) + 1e-6f
 *     sw = 0, sc = (0,0,0), sv = 0
 *     for dy in -2..2, dx in -2..2 (row-major), q = p + st*(dx,dy); skip q outside the image, invalid, or with prim[q] != prim[p]:
 *         k   = h[dy+2] * h[dx+2]
 *         x   = fabsf(Y[q] - Y[p]) / den;                    wl = 1.0f / (1.0f + x*x)
 *         d_i = albedo[q][i] - albedo[p][i];   da2 = ((d0*d0 + d1*d1) + d2*d2) + d3*d3;   wa = 1.0f / (1.0f + da2*inv_sa2)
 *         w   = (k * wl) * wa
 *         sw += w;   sc.xyz += w * c[q].xyz;   sv += (w*w) * var[q]
 *     c'[p].xyz = sc.xyz / sw;   c'[p].w = c[p].w;   var'[p] = sv / (sw*sw)
 * The centre tap always counts (sw >= 9/64); the misses form one "primitive"; the primitives are planar, so "same primitive" is an exact geometric edge
 * stop.  The weights are rational on purpose: the definition is reproducible bit for bit.  (The ideas are those of Dammertz et al. 2010 and Schied et al.
 * 2017; Y is component 1, i.e. G in SSX_MODE_RGB.) */

/* The guide buffers of the uploaded scene, row-major (row 0 = bottom): prim [height][width], depth [height][width], normal [height][width][3], albedo
 * [height][width][4]; any pointer may be NULL.  Computed by one kernel (one lane per pixel) and kept on the device per (scene upload, width, height).
 * SSX_ERR_STATE: no scene, or a render runs. */
int ssx_guides(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t* prim, float* depth, float* normal, float* albedo);
typedef struct ssx_denoise_params {
	uint32_t struct_size;  /* sizeof(ssx_denoise_params) */
	uint32_t levels;       /* L, 1..6 */
	float sigma_l, sigma_a;
} ssx_denoise_params;      /* NULL where one is expected: levels 5, sigma_l 1.0, sigma_a 0.1 (chosen on CPU renders: DESIGN.md section 12; Schied et al. publish sigma_l = 4) */
/* The filter as a pure function of its arguments (one kernel launch per level on ctx's device; needs no scene): xyza [height][width][4], var and prim
 * [height][width], albedo [height][width][4] -> xyza_out, var_out (may be NULL).  SSX_ERR_ARG: levels outside 1..6, a sigma that is not finite and
 * positive, a NULL input. */
int ssx_denoise_images(ssx_ctx* ctx, const ssx_denoise_params* params, uint32_t width, uint32_t height, const float* xyza, const float* var,
                       const uint32_t* prim, const float* albedo, float* xyza_out, float* var_out);
/* The same from the context's own state, without leaving the device: the image of the sums (what ssx_read_framebuffer returns), the variance in image units
 * from the noise estimate, the guide buffers of the scene.  xyza_out [height][width][4] and var_out [height][width] of the render's size; either may be NULL.
 * It reads only -- sums, image, noise and spectral state stay as they are, so an ssx_render_continue afterwards leaves the bits of a one-shot render -- and
 * works in SSX_MODE_RGB and with either libm.  SSX_ERR_STATE, with the reason in ssx_last_error: no scene, a render runs, no continuable sums, the noise
 * estimate off or with fewer than two batches, or a context that owns only part of the image (tile_stride != 1: combine the ranks' images and v by
 * ownership and call ssx_denoise_images).  SSX_ERR_ARG: as above. */
int ssx_denoise(ssx_ctx* ctx, const ssx_denoise_params* params, float* xyza_out, float* var_out);

/* ---- Denoising the spectral bins: extra channels under the filter's weights (appended; same ABI version) ------------------------------------------
 * As above: binary32 with IEEE + - * /, no contraction, no transcendental, in the order written, except the channel set-up, which is binary64 where said;
 * a restatement in numpy gives the same bits (tests/denoise_spectral_ref.py).
 *
 * EXTRA CHANNELS.  FILTER above is extended by E extra channels per pixel, e[p][0..E-1], 1 <= E <= 80.  At every level each extra channel of a valid p is
 * treated as c.xyz is: the same taps in the same row-major order, the same w = (k * wl) * wa,
 *     se[j] = 0;   se[j] += w * e[q][j] for every tap q that is not skipped;   e'[p][j] = se[j] / sw
 * A skipped tap (outside the image, invalid, or of another primitive) is skipped, not added with weight 0: 0 * inf is NaN.  An invalid p keeps its e at
 * every level.  A non-finite e[q][j] of a counted tap goes through the arithmetic as it is: validity is decided by X, Y, Z and var only.  The weights never
 * depend on e; c' and var' are those of FILTER, bit for bit.
 *
 * SPECTRAL CHANNELS.  n = ssx_done_spp, B bins, M = B / 4, S and N the sums and counts of "Spectral radiance output"; E = B + M:
 *     e0[p][b]     = (float)(S[p][b] / (double)n)            b = 0..B-1   (binary64 division, then rounded)
 *     e0[p][B + m] = (float)((double)N[p][m] / (double)n)    m = 0..M-1
 *     eL = e0 after the L levels
 *     out[p][b] = eL[p][B + b%M] > 0 ? eL[p][b] / eL[p][B + b%M] : 0.0f
 * out is a ratio of filtered sums to filtered counts: every neighbour's bin enters with the number of samples behind it, the inverse-variance weight of a
 * mean of N samples, and the weighting composes linearly across the levels.  A bin without a sample at p is filled from the neighbours that have some
 * (filtering mean[p][b] itself would average their values with the zeros of the empty bins). */

/* FILTER with E = channels extra channels as a pure function of its arguments (needs no scene): the inputs of ssx_denoise_images, and extra -> extra_out,
 * both row-major [height][width][E].  xyza_out and var_out may be NULL and are those of ssx_denoise_images; extra and extra_out may not.  On the device the
 * channels lie in groups of four (two ping-pong buffers of ceil(E / 4) * width * height * 16 bytes); every level is one more kernel launch next to the
 * filter's.  SSX_ERR_ARG: as ssx_denoise_images; channels outside 1..80; a NULL extra or extra_out; an image at which one of those channel buffers would
 * exceed 2 GiB (2^31 bytes). */
int ssx_denoise_channels(ssx_ctx* ctx, const ssx_denoise_params* params, uint32_t width, uint32_t height, const float* xyza, const float* var,
                         const uint32_t* prim, const float* albedo, uint32_t channels, const float* extra /* [H][W][E] */,
                         float* xyza_out, float* var_out, float* extra_out /* [H][W][E] */);
/* SPECTRAL CHANNELS from the context's own state, without leaving the device: mean_out [height][width][B] receives `out`, xyza_out and var_out what
 * ssx_denoise returns; any of the three may be NULL.  The rules of ssx_denoise, and one more: spectral output must be on and the context must hold valid
 * bins (after ssx_sums_import without ssx_spectral_import it holds none) -- otherwise SSX_ERR_STATE with the reason in ssx_last_error.  It reads only: image, sums, noise and spectral
 * state stay as they are, so an ssx_render_continue afterwards leaves the bits of a one-shot render in the image and in ssx_spectral_read. */
int ssx_denoise_spectral(ssx_ctx* ctx, const ssx_denoise_params* params, float* mean_out /* [H][W][B] */, float* xyza_out, float* var_out);

/* ---- Developing the spectral bins: observers, filters, sensors (appended; same ABI version) -------------------------------------------------------
 * The way back from the bins, raw or denoised, to a colour image: one linear map per pixel from B bins to C output channels, so that a render can be viewed
 * under another observer, through a colour filter, with a camera's response curves or under another illuminant without rendering again.  The definition is
 * this library's; a restatement in numpy gives the same bits (tests/develop_ref.py).
 *
 * DEVELOP.  Per pixel p, B values q[p][b] (B in {4, 8, ..., 64}) and a weight matrix W[c][b], C output channels, 1 <= C <= 16:
 *     out[p][c] = sum over b of q[p][b] * W[c][b]
 * in binary32: acc = 0.0f, then acc = acc + (q[p][b] * W[c][b]) for b = 0, 1, ..., B-1 -- the product is rounded before the add, no contraction, no
 * reassociation.  Non-finite values go through the arithmetic as they are.
 *
 * SOURCES OF q.
 *   raw       from the context's state, n = ssx_done_spp, M = B / 4, S the sums of "Spectral radiance output":
 *                 q[p][b] = (float)((S[p][b] * (double)M) / (double)n)        the multiply, then the divide, both binary64
 *             This is NOT mean[p][b]: at 16 spp and 64 bins a third of the sub-bins hold no sample and mean reads 0 there.  S * M / n is the estimator the
 *             integrator itself uses for the pixel (every sample counts once; the sub-bin of a sample is drawn uniformly among M, so each holds n / M in
 *             expectation), with the observer replaced by its average over the bin: an empty sub-bin costs nothing and biases nothing.  Pixels the context
 *             does not own read +0 in every channel.
 *   denoised  q[p][b] = out[p][b] of ssx_denoise_spectral (the ratio of "Denoising the spectral bins") for the same parameters.
 *   caller's  any [height][width][B] float array, through ssx_develop_images.
 *
 * WEIGHTS are built on the host (libssx_host.so ssh_develop_weights, include/ssx_host.h), in binary64, and rounded to binary32 once at the end.  A tabulated
 * spectrum T -- n samples s_0 .. s_(n-1) over [low, high] -- is the function the host Spectrum's linear sampler evaluates, restated in binary64:
 *     delta = ((double)high - (double)low) / (n - 1);   pos = (lambda - (double)low) / delta;   i = floor(pos);   f = pos - i
 *     T(lambda) = s(i) * (1.0 - f) + s(i + 1) * f,      s(k) = (double)s_k for 0 <= k < n and 0 otherwise
 * OUTSIDE THE TABLE'S RANGE the sampler does not clamp: the table runs linearly to zero over one step beyond either end (knots low - delta and high + delta
 * carry the value 0) and is zero beyond.  T is piecewise linear with knots low + k * delta, k = -1 .. n.
 * Bin b covers [e_b, e_(b+1)], e_b = (double)lambda_min + b * ((double)lambda_step / M).  For response curves r_c, an optional filter g (a missing g is 1) and an
 * optional gain per bin (a missing one is 1):
 *     I[c][b] = integral over [e_b, e_(b+1)] of r_c(lambda) * g(lambda) dlambda;        W[c][b] = (float)(gain[b] * I[c][b])
 * integrated exactly, piecewise: the breakpoints are e_b, e_(b+1) and every knot of either table strictly between them, sorted, equal ones taken once; on each
 * piece [a, z] the integrand is a quadratic at most, so Simpson's rule is exact: ((z - a) / 6.0) * ((F(a) + 4.0 * F(0.5 * (a + z))) + F(z)), F = r_c * g (or
 * r_c); the pieces are added in ascending order starting from 0.0.  The bin's width is inside W: q is flux per nm and out has the units of the XYZ image.
 * Output space: xyz -- the weights as integrated; lrgb -- the host's XYZ -> BT.709 matrix m (ssh_color_values "xyz_to_lrgb", column-major) applied to the three
 * rows in binary64 before the rounding: (m[0][r] * X + m[1][r] * Y) + m[2][r] * Z with X, Y, Z = gain[b] * I[0..2][b].
 * RELIGHTING.  relight_gain(old, new)[b] = (integral of new over bin b) / (integral of old over bin b), 0 where the integral of old is 0 (ssh_relight_gain);
 * it is passed as the gain.  This is exact only when every emitter of the scene carries `old` up to a scale -- all light then has the factor old(lambda) -- and
 * only up to the variation of new / old inside a bin.
 *
 * ON THE DEVICE the map is one memory-bound kernel: one wave per owned 8x8 tile (raw; it reads S[tile slot][bin][pixel of the tile], 512 consecutive bytes
 * per bin) or one lane per pixel (images), the weights read at wave-uniform addresses from a buffer of at most 4 KB, up to 16 accumulators in registers.
 * With the feature unused nothing is allocated and nothing is launched. */

/* DEVELOP as a pure function of its arguments (needs no scene): q [height][width][bins], weights [channels][bins] -> out [height][width][channels], all
 * row-major floats.  SSX_ERR_ARG: channels outside 1..16, bins not a multiple of 4 in 4..64, a NULL pointer, an empty or too large image. */
int ssx_develop_images(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const float* q /* [H][W][B] */, const float* weights /* [C][B] */,
                       uint32_t channels, float* out /* [H][W][C] */);
/* DEVELOP from the context's own state, without the bins leaving the device: denoise == NULL selects the raw source, otherwise the denoised source with these
 * parameters (the filter runs as in ssx_denoise_spectral and its ratio is developed where it lies).  out: [height][width][channels] of the render's size, row
 * 0 = bottom (NULL: the kernels run and the result stays on the device -- for measurements).  It reads only: image, sums, noise and spectral state stay as they are, so an
 * ssx_render_continue afterwards leaves the bits of a one-shot render in the image and in ssx_spectral_read.  SSX_ERR_STATE, with the reason in
 * ssx_last_error: spectral output is off, a render runs, the context holds no valid bins (nothing rendered, or ssx_sums_import alone, or a changed bin count),
 * ssx_done_spp == 0, and, for the denoised source, whatever ssx_denoise_spectral refuses.  SSX_ERR_ARG: channels outside 1..16, a NULL weights. */
int ssx_spectral_develop(ssx_ctx* ctx, const ssx_denoise_params* denoise, const float* weights /* [C][B] */, uint32_t channels, float* out /* [H][W][C] */);

/* ---- Demodulated denoising: the filter on illumination, the albedo divided out per bin (appended; same ABI version) ---------------------------------
 * The filter of Schied et al. runs on illumination -- radiance divided by the first-hit albedo -- and multiplies the albedo back afterwards; on a textured
 * surface every texel boundary is otherwise a luminance edge and the filter averages texels of like colour only.  A spectral renderer knows the albedo per
 * wavelength, and the bins of "Spectral radiance output" are aligned with the hero slots, so the bins are demodulated exactly, bin by bin.  The definition is
 * this library's.  Binary32 with IEEE + - * /, no contraction, in the order written; a restatement in numpy gives the same bits (tests/demod_ref.py).
 *
 * ALBEDO BINS.  rho[p][b] for every pixel p = (i, j) of a width x height image, B bins (B in {4, 8, ..., 64}, M = B / 4) and K in {1, 2, 4} rays per axis;
 * independent of seed, spp and ownership; refused in SSX_MODE_RGB, as spectral output is.
 *     acc[0..B-1] = 0
 *     for c = 0..K-1 (outer), a = 0..K-1 (inner): the ray through ((double)i + ((double)a + 0.5) / K, (double)j + ((double)c + 0.5) / K) -- camera_dir, normalised and
 *         rounded to float and traced exactly as a ray of GUIDE BUFFERS is -- and for m = 0..M-1:
 *             lambda_0 = lambda_min + ((float)m + 0.5f) * (lambda_step / (float)M)
 *             al = what the device function behind SSX_DBG_ALBEDO returns for (prim, st of the hit, lambda_0); +0 in all four components for a miss
 *             acc[i*M + m] = acc[i*M + m] + al[i]     (i = 0..3)
 *     rho[p][b] = acc[b] / (float)(K*K)
 * At K = 1, B = 4 rho is the albedo of GUIDE BUFFERS bit for bit (lambda_0 is lambda_g).
 *
 * CHANNEL ALBEDO.  Given weights Wc[3][B] (X, Y, Z rows; the hosts default them to the develop weights of the render's own observer):
 *     num[p][c] = DEVELOP of rho[p][.] with Wc[c][.];   den[c] = the same accumulation with every q = 1.0f;   rho_c[p][c] = num[p][c] / den[c]
 * den[c] <= 0 (or NaN) is refused.
 *
 * DEMODULATE.  f = albedo_floor;  r~[p][b] = rho[p][b] > f ? rho[p][b] : f;  r~_c[p][c] likewise from rho_c.  valid(p) as in FILTER, of the inputs c and var.  For a
 * valid p, with e0 the SPECTRAL CHANNELS:
 *     e0'[p][b] = e0[p][b] / r~[p][b]   (b = 0..B-1; the M count channels stay);   c'[p][k] = c[p][k] / r~_c[p][k]   (k = X, Y, Z; alpha stays)
 *     var'[p] = var[p] / (r~_c[p][1] * r~_c[p][1])
 * An invalid p keeps e0, c and var, and is not remodulated either: it passes through the whole mode untouched.
 * Below the floor a dark texel is under-demodulated and darkens its neighbours' estimate; above it the mode stops doing anything.
 *
 * FILTER.  FILTER with EXTRA CHANNELS, unchanged, on c', var', e0', with the scene's prim guide and an ALL-ZERO albedo guide: wa = 1.0f / (1.0f + 0.0f) is exactly
 * 1 -- the demodulation replaces the albedo stop.  sigma_a is IGNORED in this mode (any value, also an invalid one, is accepted).
 *
 * REMODULATE.  With cL, varL, eL the filter's results, for a p that was valid on input:
 *     out[p][b]   = eL[p][B + b%M] > 0 ? (eL[p][b] / eL[p][B + b%M]) * r~[p][b] : 0.0f
 *     c_out[p][k] = cL[p][k] * r~_c[p][k]   (alpha stays);      var_out[p] = varL[p] * (r~_c[p][1] * r~_c[p][1])
 * and without the multiplications for a p that was not. */

/* rho_out [height][width][bins], row-major (row 0 = bottom); NULL: computed and kept only.  Two kernels: the albedo kernel (one lane per pixel and pair of sub-bins m; an
 * odd M: per sub-bin; on the device the bins lie planar in groups of four, float4 [bins / 4][height][width], the layout of the filter's channel buffers) and the
 * copy into the row-major array returned here; cached per (scene upload, width, height, bins, supersample) and
 * dropped by ssx_upload_scene, as the guide buffers are.  SSX_ERR_STATE: no scene, a render runs, a scene in SSX_MODE_RGB.  SSX_ERR_ARG: bins not a multiple of
 * 4 in 4..64, supersample not 1, 2 or 4, an empty or too large image. */
int ssx_albedo_bins(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, uint32_t supersample, float* rho_out /* [H][W][B] */);
#define SSX_DEMOD_DEFAULT_FLOOR 0.0625f  /* 1/16 */
#define SSX_DEMOD_DEFAULT_SIGMA_L 1.0f
typedef struct ssx_demod_params {
	uint32_t struct_size;  /* sizeof(ssx_demod_params) */
	uint32_t supersample;  /* K: 1, 2 or 4 */
	float albedo_floor;    /* finite and positive */
} ssx_demod_params;        /* NULL where one is expected: supersample 2, albedo_floor SSX_DEMOD_DEFAULT_FLOOR (chosen on CPU renders: DESIGN.md section 15) */
/* ssx_denoise_spectral in this mode, from the context's own state and without leaving the device: mean_out [height][width][B] receives `out`, xyza_out c_out,
 * var_out var_out; any of the three may be NULL.  params == NULL: levels 5, sigma_l SSX_DEMOD_DEFAULT_SIGMA_L (the mode's own default: DESIGN.md section 15).
 * weights_xyz is Wc.  The state rules of ssx_denoise_spectral: it reads only -- image, sums, noise and spectral state stay as they are, so an ssx_render_continue
 * afterwards leaves the bits of a one-shot render -- and refuses what that refuses.  SSX_ERR_ARG also: a NULL weights_xyz, a row of it whose den is not positive,
 * supersample or albedo_floor out of range.  (A scene in SSX_MODE_RGB never holds valid bins.) */
int ssx_denoise_spectral_demod(ssx_ctx* ctx, const ssx_denoise_params* params, const ssx_demod_params* demod, const float* weights_xyz /* [3][B] */,
                               float* mean_out /* [H][W][B] */, float* xyza_out, float* var_out);
/* ssx_spectral_develop with this mode's `out` as the source q: the remodulated bins are developed where they lie.  weights [channels][B] and out as there. */
int ssx_spectral_develop_demod(ssx_ctx* ctx, const ssx_denoise_params* denoise, const ssx_demod_params* demod, const float* weights_xyz /* [3][B] */,
                               const float* weights /* [C][B] */, uint32_t channels, float* out /* [H][W][C] */);

/* ---- Spectral moments and region probes: error bars for the bins (appended; same ABI version) --------------------------------------------------------
 * A bin mean of "Spectral radiance output" comes without an uncertainty, and the per-sample fluxes exist only between one launch and the next.  With the
 * moments on, the sample walk keeps a per-pixel, per-bin second moment of the hero fluxes beside the sums S.  The samples of a pixel have independent
 * streams (the seeding contract above), so a plain sample variance inside each sub-bin is the estimator; no batch means are needed.  Everything below is
 * binary64 with IEEE + - * / only, no contraction, the operations in the order written: a restatement in numpy gives the same bits
 * (tests/spectral_stats_ref.py).
 *
 * SECOND MOMENT.  With m, i, f[i] as there, for sample k of pixel p, in ascending k:
 *       Q[p][i*M + m] += (double)f[i] * (double)f[i]          (the product is exact in binary64)
 *   Q has the shape and the device layout of S; a non-finite flux is added as it is; the counts are N.
 * VARIANCE OF A BIN MEAN.  For bin b, with n = N[p][b % M]:
 *       n < 2 :  var[p][b] = +inf (binary32)                  unknown, not zero
 *       else  :  q = Q - (S*S) / (double)n;   q = (q < 0.0) ? 0.0 : q         (a NaN stays a NaN)
 *                var[p][b] = (float)((q / (double)(n-1)) / (double)n)
 *   Pixels the context does not own read as 0 (var and Q).
 * PROBE.  labels: uint8 [height][width], row 0 = bottom; 0..R-1 names a region (R <= 32), 255 none, any other value is SSX_ERR_ARG.  For region r and bin
 *   b, with m = b % M, over the pixels p labelled r (n_p = N[p][m], q_p as above):
 *       SS = sum S[p][b]                NN = sum n_p                                          (uint64)
 *       VV = sum over n_p >= 2 of (q_p / (double)(n_p - 1)) * (double)n_p
 *       UU = sum over n_p < 2 of n_p                                                          (uint64: samples whose variance is unestimated)
 *   The order of the binary64 additions is part of the definition: within a row the pixels are added in ascending i starting from +0.0, one partial per row;
 *   the row partials are added in ascending j starting from +0.0; a row without a pixel of the region contributes its +0.0.  The four arrays are [R][B];
 *   NN and UU are repeated over i like the counts.  The hosts derive
 *       mean = NN ? SS / NN : 0          stderr = sqrt(VV * NN / (NN - UU)) / NN               (NaN when NN - UU == 0)
 *   Conditional on the counts Var(sum S_p) = sum n_p sigma_p^2, and q_p / (n_p - 1) is unbiased for sigma_p^2; the samples in sub-bins too thin to estimate
 *   (UU of them) are taken to have the average variance of the others.  The pooled mean weights samples, not pixels.
 * The state follows the bins' rule -- valid from zero samples or not at all: a sample-walking ssx_render_start resets it, ssx_render_continue carries it on,
 * whatever clears the bins clears it, and it is invalid when it is switched on over existing bins.  ssx_spectral_import ALONE leaves the moments invalid: it does
 * not carry Q -- a continue then renders normally, bins included, and the read calls below return SSX_ERR_STATE with the reason; ssx_spectral_moments_import,
 * called on top of it with the Q of the same samples, makes them valid again, so that a checkpoint which carries Q (libssx_host.so: "SSXCKPT3") resumes with
 * its error bars and its stopping rule.  Image, sums and bins of a render do not depend on whether the moments are on. */

/* enable: 0 = off (default: nothing allocated, nothing launched), else on: the sample walk runs one more small kernel per launch, which reads the launch's
 * fluxes again, and the context holds Q (as large as S; ssx_scratch_info counts it with the sample arrays).  Needs spectral output on (SSX_ERR_STATE; switching
 * the bins off switches the moments off); not while a render runs (SSX_ERR_STATE). */
int ssx_set_spectral_moments(ssx_ctx* ctx, int enable);
/* Row-major (row 0 = bottom) var [height][width][B] (float) and q [height][width][B] (the binary64 accumulators Q); either may be NULL.  info is filled as
 * by ssx_spectral_read.  SSX_ERR_STATE: spectral output or the moments are off, a render runs, or the context holds no valid bins or moments. */
int ssx_spectral_variance(ssx_ctx* ctx, ssx_spectral_info_t* info, float* var, double* q);
/* The inverse of ssx_spectral_variance(q), for a checkpoint: the context takes, from the whole-image array q [height][width][B] (row-major, row 0 = bottom), the
 * tiles it owns under its current parameters -- whoever exported it may have owned other tiles, as long as the array holds every pixel this context owns (merge
 * the ranks' exports by ownership first).  One kernel, a transposition through LDS per owned 8x8 tile; tile lanes outside a ragged image receive +0.0.
 * Valid only DIRECTLY ON TOP OF a successful ssx_spectral_import: spectral output and the moments are on, the bins are valid and came from that call, and nothing
 * has rendered since (ssx_set_spectral_moments(1) may come before or after the two imports underneath).  On success the context is what it would be had it
 * rendered the ssx_done_spp samples with the moments on: ssx_render_continue carries Q on; ssx_spectral_variance, ssx_spectral_probe and ssx_spectral_noise work.
 * The same kernel checks what it takes against the context's own S and N, with rules that hold exactly for everything the moment kernel can produce (Q +=
 * (double)f * (double)f from +0.0, every product exact), per owned in-image pixel and bin, n = N[p][b % M]:
 *       n == 0 :  Q is +0.0, bit for bit
 *       n == 1 :  Q == S * S, or both are NaN
 *       n >= 2 :  !(Q < 0.0)
 *   They catch the Q of another render, one rank's unmerged export (zeros against n > 0 pass the third rule but mostly fail the second at low sample counts)
 *   and S handed in as Q; they cannot vouch for values at n >= 2 -- the file's checksum does that.  No inexact rule is applied.
 * SSX_ERR_STATE: spectral output or the moments are off, a render runs, or there is no such import underneath.  SSX_ERR_ARG, ssx_last_error naming the field or
 * the rule: a NULL pointer, struct_size; width or height differ from the context's; info->bins from its bin count; info->done_spp from ssx_done_spp; lambda_min
 * or bin_width, compared as bits, from the uploaded scene's; the check fails.  After a refusal the moments are invalid; bins and pixel sums are untouched: a
 * continue renders normally.  done_spp == 0 is legal (q all +0.0).  Q is reserved for the owned tiles before the kernel runs (ssx_scratch_info counts it). */
int ssx_spectral_moments_import(ssx_ctx* ctx, const ssx_spectral_info_t* info, const double* q /* [H][W][B] */);
/* The probe of the context's own state: it exports S, Q and N row-major to device temporaries and runs the kernels of ssx_probe_arrays on them -- the same
 * bits.  Pixels the context does not own add nothing.  SS, NN, VV, UU: [regions][B].  It reads only.  SSX_ERR_STATE as ssx_spectral_variance; SSX_ERR_ARG: a
 * NULL argument, regions outside 1..32, a label that is neither a region nor 255. */
int ssx_spectral_probe(ssx_ctx* ctx, const uint8_t* labels /* [H][W] */, uint32_t regions, double* SS, uint64_t* NN, double* VV, uint64_t* UU);
/* The same probe as a pure function of its arguments (no scene needed, like ssx_denoise_images): sums and q [height][width][bins], counts
 * [height][width][bins / 4] -- e.g. several devices' exports merged by ownership.  Two kernels: one workgroup per image row walks it in ascending i, then one
 * lane per region and bin adds the rows in ascending j. */
int ssx_probe_arrays(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const double* sums, const double* q, const uint32_t* counts,
                     const uint8_t* labels /* [H][W] */, uint32_t regions, double* SS, uint64_t* NN, double* VV, uint64_t* UU);

/* ---- Spectral noise figure: when are the bins converged (appended; same ABI version) -----------------------------------------------------------------
 * The error bars above, reduced to one number per image or masked region, for a render loop that stops on it (the hosts' render_until_spectral) -- the analogue
 * for the bins of the batch-means figure of component Y.  Binary64 with IEEE + - * / only, no contraction, the operations in the order written, as above: a
 * restatement in numpy gives the same bits (tests/spectral_noise_ref.py).  Notation as above.
 *
 * PER PIXEL.  For an owned in-image pixel p and bin b, with m = b % M, n = N[p][m] and q as in VARIANCE OF A BIN MEAN:
 *       n >= 2 (estimable)   :  e = (q / (double)(n-1)) / (double)n      the variance of the bin mean, before its rounding to binary32
 *                               mu = S[p][b] / (double)n
 *       n <  2 (unestimated) :  the pixel contributes to neither sum
 * MASK.  uint8 [height][width], row 0 = bottom; NULL means every pixel, a nonzero value that the pixel is in.
 * PER 8x8 TILE.  For tile t = ty * tiles_x + tx (tiles_x = (width + 7) / 8) and bin b, over the tile's in-image, in-mask pixels in ascending row, then ascending
 *   column, every binary64 partial starting from +0.0:
 *       EV_t[b] = sum of e  over the estimable pixels          PP_t[b] = the number of estimable pixels     (uint32)
 *       EM_t[b] = sum of mu over the estimable pixels          PU_t[b] = the number of unestimated pixels   (uint32)
 * IMAGE.  EV[b], EM[b], PP[b], PU[b] (the counts uint64): the tile partials added in ascending t, from +0.0 / 0.  A tile the context does not own contributes
 *   +0.0 and 0.
 *   THIS IS BIT-NEUTRAL, and it is why the partials are per tile -- the unit of ownership -- and not per image row, which several devices share: a partial that
 *   started from +0.0 is never -0.0 (in round-to-nearest a sum is -0.0 only when both operands are), and x + (+0.0) == x for every x other than -0.0; a NaN
 *   stays a NaN.  So adding a foreign tile's +0.0 changes no bit of the running total.  Several devices' tile partials are
 *   therefore merged by ownership -- tile t from the device that owns it -- and reduced in the same ascending order by ssx_spectral_noise_reduce: the totals have
 *   the bits of one device that owned every tile.  (Row partials would have to ADD the devices' shares of a row, in another order than one device adds them.)
 * DERIVED BY THE HOSTS (ssh_spectral_noise_derive, include/ssx_host.h).  With P = sum over b of PP[b], U = sum over b of PU[b], EVs = sum of EV[b], EMs = sum of
 *   EM[b], every sum over ascending b from +0.0 / 0, and mean = EMs / (double)P:
 *       noise    = sqrt(EVs / (double)P) / mean        NaN when P == 0 or mean == 0
 *       coverage = (double)P / (double)(P + U)         NaN when P + U == 0 (an empty mask)
 *       rel[b]   = sqrt(EV[b] / PP[b]) / (EM[b] / PP[b])   per bin, NaN when PP[b] == 0 or the bin's mean is 0
 *   noise is the RMS standard error of the pixels' bin means relative to the mean bin flux.  The unestimated sub-bins are taken to have the others' average
 *   variance (the assumption behind UU above); coverage says how many there are.  A non-finite flux makes the figure NaN, and NaN <= target is false: such a
 *   render runs to its sample cap, as does one whose mask is empty.
 *
 * ON THE DEVICE: ssx_spectral_noise_tiles_kernel, one workgroup per owned tile slot, reads S, Q and N where they lie -- [slot][bin][64], [slot][m][64]; no
 * export to row-major, no temporary of the image's size: the stage buffer holds the mask and the [tiles][B] partials -- and writes the four partials at the
 * tile's image index t; ssx_spectral_noise_reduce_kernel, one lane per (quantity, bin), walks t in ascending order.  No atomics. */

/* The figure of the context's own state.  mask: [height][width] or NULL.  EV, EM (binary64), PP, PU (uint64): [B].  tEV, tEM (binary64), tPP, tPU (uint32):
 * [tiles][B], tiles = ((width + 7) / 8) * ((height + 7) / 8), the tile partials; each of the four may be NULL.  It reads only: image, sums, bins and moments stay
 * as they are, so an ssx_render_continue afterwards leaves the bits of a render that was never asked.  SSX_ERR_STATE, with the reasons of ssx_spectral_variance:
 * spectral output or the moments are off, a render runs, or the context holds no valid bins or moments (after ssx_spectral_import, a changed bin count, ...).
 * SSX_ERR_ARG: a NULL EV, EM, PP or PU. */
int ssx_spectral_noise(ssx_ctx* ctx, const uint8_t* mask /* [H][W] or NULL */, double* EV, double* EM, uint64_t* PP, uint64_t* PU /* [B] */,
                       double* tEV, double* tEM, uint32_t* tPP, uint32_t* tPU /* [tiles][B], each may be NULL */);
/* IMAGE as a pure function of its arguments (no scene needed, like ssx_probe_arrays): the second kernel on uploaded tile partials -- e.g. several devices'
 * partials merged by ownership.  SSX_ERR_ARG: bins not a multiple of 4 in 4..64, tiles outside 1..2^22, a NULL pointer.  SSX_ERR_STATE: a render runs. */
int ssx_spectral_noise_reduce(ssx_ctx* ctx, uint32_t tiles, uint32_t bins, const double* tEV, const double* tEM, const uint32_t* tPP, const uint32_t* tPU /* [tiles][bins] */,
                              double* EV, double* EM, uint64_t* PP, uint64_t* PU /* [bins] */);

/* ---- Comparing two spectral renders: bin by bin, with error bars and z-scores (appended; same ABI version) -------------------------------------------
 * Two renders of one view -- two uplifts, two observers, two versions of the code -- differ somewhere; whether the difference exceeds the noise is a question
 * for S, Q and N of both.  The probes give the difference of two pooled means; they cannot see a structured difference that cancels inside the region, and they
 * give no per-pixel map.  Binary64 with IEEE + - * / only, no contraction, the operations in the order written, no square root on the device (the hosts take
 * roots): a restatement in numpy gives the same bits (tests/spectral_compare_ref.py).  Notation as above.
 *
 * INPUTS.  Two array sets X in {A, B}, row-major, row 0 = bottom: S_X, Q_X double [height][width][B], N_X uint32 [height][width][M], B in {4, 8, ..., 64}, M = B /
 *   4; width, height and B are those of both sets, the sample counts may differ (the normal case).  labels as in PROBE (R <= 32, 255: none).  t2: the squared z
 *   threshold, finite and >= 0.
 * PER CELL.  For pixel p and bin b, with m = b % M and nX = N_X[p][m]: the cell is COMPARABLE iff nA >= 2 && nB >= 2.  For a comparable cell, with qX, eX =
 *   (qX / (double)(nX-1)) / (double)nX and muX = S_X[p][b] / (double)nX exactly as in "Spectral noise figure", PER PIXEL:
 *       d  = muA - muB
 *       v  = eA + eB
 *       z2 = (v == 0.0 && d == 0.0) ? 0.0 : (d * d) / v
 *   The special case is two black cells (samples that hit nothing count with f = 0: common): they agree, and must not produce a NaN.  v == 0 with d != 0 gives
 *   +inf as IEEE gives it; a NaN stays a NaN.
 * MAPS (optional, every pixel, labelled or not).  diff [height][width][B] float: (float)d for a comparable cell, 0.0f otherwise.  var [height][width][B] float:
 *   (float)v for a comparable cell, +inf otherwise -- unknown, not zero, as in VARIANCE OF A BIN MEAN.
 * PER REGION r AND BIN b, over the pixels labelled r, six arrays [R][B]:
 *       DD = sum d      VV = sum v      X2 = sum z2             over the comparable cells, binary64
 *       CC = the number of comparable cells        NC = the number of not-comparable cells        EX = the number of comparable cells with z2 > t2      (uint64)
 *   The comparison is strict: a NaN does not count.  The order of the binary64 additions is PROBE's and part of the definition: within a row ascending i from
 *   +0.0, one partial per row; the row partials in ascending j from +0.0; a row without a pixel of the region contributes its +0.0.
 * DERIVED BY THE HOSTS (ssh_compare_derive, include/ssx_host.h), each NaN where its denominator is 0:
 *       mean_diff = DD / CC        stderr = sqrt(VV) / CC        z = DD / sqrt(VV)        chi2 = X2 / CC        exceed = EX / CC        coverage = CC / (CC + NC)
 *   and the per-pixel signed map zmap = diff / sqrt(var), 0 where var is +inf.  stderr uses that the pixels are independent.
 * WHAT THE NUMBERS MEAN.  The model is Welch's: d / sqrt(v) with the two variances estimated separately, and the two renders must have INDEPENDENT samples.  With
 *   few samples per sub-bin z2 is the square of a t-like variable with nu degrees of freedom (Welch-Satterthwaite), and under equality E[z2] = nu / (nu - 2),
 *   not 1: chi2 is to be held against that, and no p-values are promised.  Two renders with the SAME SEED are positively correlated: v then overstates the variance
 *   of d and every z is too small.  The fluxes are not Gaussian either: at a few samples per sub-bin the figures are indications.
 *
 * ON THE DEVICE: ssx_compare_rows_kernel, one workgroup per image row, classifies a chunk of the row 256 lanes wide -- reads and map writes contiguous across
 * the lanes, every byte of S and Q fetched once -- stages d, v, z2 in LDS and walks the chunk in ascending i with one lane per (quantity pair, bin), the
 * accumulators in LDS indexed by the label; ssx_compare_reduce_kernel, one lane per (quantity, r, b), walks j in ascending order.  No atomics. */

/* The comparison as a pure function of its arguments (no scene needed, like ssx_probe_arrays): e.g. two checkpoints' arrays, or several devices' exports merged
 * by ownership.  DD, VV, X2 (binary64), CC, NC, EX (uint64): [regions][bins].  diff, var: [height][width][bins] float, either may be NULL.  SSX_ERR_ARG, with
 * ssx_last_error naming the field: bins not a multiple of 4 in 4..64, an empty or too large image, a NULL required pointer, regions outside 1..32, a label that is
 * neither a region nor 255, a t2 that is negative, infinite or NaN.  SSX_ERR_STATE: a render runs. */
int ssx_spectral_compare_arrays(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const double* SA, const double* QA, const uint32_t* NA,
                                const double* SB, const double* QB, const uint32_t* NB, const uint8_t* labels /* [H][W] */, uint32_t regions, double t2,
                                double* DD, double* VV, double* X2, uint64_t* CC, uint64_t* NC, uint64_t* EX, float* diff, float* var);
/* A is the context's own state: it exports S, Q and N row-major to device temporaries, as ssx_spectral_probe does, and runs the kernels of
 * ssx_spectral_compare_arrays on them -- the same bits.  Pixels the context does not own have count 0 and are not comparable.  other_info describes B (what
 * ssx_spectral_read or a checkpoint said of it).  It reads only: image, sums, bins and moments stay as they are, so an ssx_render_continue afterwards leaves the
 * bits of a render that was never asked.  SSX_ERR_STATE, with the reasons of ssx_spectral_variance: spectral output or the moments are off, a render runs, or the
 * context holds no valid bins or moments.  SSX_ERR_ARG, naming the field: other_info NULL or differing from the context in struct_size, width, height, bins, or in
 * lambda_min or bin_width compared as bits (done_spp may differ); and what ssx_spectral_compare_arrays refuses. */
int ssx_spectral_compare(ssx_ctx* ctx, const ssx_spectral_info_t* other_info, const double* SB, const double* QB, const uint32_t* NB, const uint8_t* labels /* [H][W] */,
                         uint32_t regions, double t2, double* DD, double* VV, double* X2, uint64_t* CC, uint64_t* NC, uint64_t* EX, float* diff, float* var);

/* ---- Colour difference of two developments: CIELAB, dE*ab and CIEDE2000 maps with region figures (appended; same ABI version) ---------------------------
 * Two developments of one render -- two observers, raw against denoised, a relight against a re-render -- differ somewhere; whether the difference can be SEEN
 * is not a question for the bins (a 3-sigma difference in one bin may be invisible, a visible hue shift may be spread over bins so that none is significant)
 * but for a colour-difference formula on the developed images.  The definition is this library's; tests/delta_e_ref.py restates it in numpy.
 *
 * INPUTS PER PIXEL.  Two XYZ triples A, B in binary32 (DEVELOP with C = 3 in the xyz space), two reference whites wA[3], wB[3] in binary64, every component
 *   finite and > 0.  labels as in PROBE (R <= 32, 255: none); labels NULL: the whole image is region 0, R = 1.  Two thresholds t[2], finite and >= 0.
 * LAB.  Per side, binary64, with x = (double)X / w[0], y = (double)Y / w[1], z = (double)Z / w[2]:
 *       f(u) = cbrt(u) for u > 216.0 / 24389.0 ((6/29)^3), else u / (108.0 / 841.0) + 4.0 / 29.0            (108/841 = 3 (6/29)^2)
 *       L = 116.0 * f(y) - 16.0        a = 500.0 * (f(x) - f(y))        b = 200.0 * (f(y) - f(z))
 *   Negative and non-finite inputs go through as the arithmetic gives them (a NaN fails the comparison and takes the line).
 * dE*ab.  dL = L_A - L_B, da = a_A - a_B, db = b_A - b_B;  dEab = sqrt((dL * dL + da * da) + db * db).
 * dE00.  CIEDE2000 with kL = kC = kH = 1 as Sharma, Wu and Dalal state it (Color Res. Appl. 30 (2005) 21-30); 1 is side A, 2 is side B, angles in degrees, rad
 *   = 0.017453292519943295, deg = 57.29577951308232, p7(c) = (((c * c) * (c * c)) * (c * c)) * c, K = 6103515625.0 (25^7):
 *       C_i  = sqrt(a_i * a_i + b_i * b_i)                         m7 = p7(0.5 * (C_1 + C_2))              G = 0.5 * (1.0 - sqrt(m7 / (m7 + K)))
 *       a'_i = (1.0 + G) * a_i                                     C'_i = sqrt(a'_i * a'_i + b_i * b_i)
 *       h'_i = 0 where a'_i == 0 && b_i == 0; else h = atan2(b_i, a'_i) * deg, and h + 360.0 where h < 0.0
 *       dL' = L_2 - L_1        dC' = C'_2 - C'_1        P = C'_1 * C'_2        d = h'_2 - h'_1        s = h'_1 + h'_2        far = |h'_1 - h'_2| > 180.0
 *       dh' = 0.0 where P == 0.0;  else d where !far;  else d - 360.0 where d > 180.0;  else d + 360.0
 *       dH' = (2.0 * sqrt(P)) * sin((0.5 * dh') * rad)
 *       Lm = 0.5 * (L_1 + L_2)        Cm = 0.5 * (C'_1 + C'_2)
 *       hm = s where P == 0.0;  else 0.5 * s where !far;  else 0.5 * (s + 360.0) where s < 360.0;  else 0.5 * (s - 360.0)
 *       T  = (((1.0 - 0.17 * cos((hm - 30.0) * rad)) + 0.24 * cos((2.0 * hm) * rad)) + 0.32 * cos((3.0 * hm + 6.0) * rad)) - 0.20 * cos((4.0 * hm - 63.0) * rad)
 *       u  = (hm - 275.0) / 25.0        dtheta = 30.0 * exp(-(u * u))        c7 = p7(Cm)        RC = 2.0 * sqrt(c7 / (c7 + K))
 *       l  = (Lm - 50.0) * (Lm - 50.0)  SL = 1.0 + (0.015 * l) / sqrt(20.0 + l)        SC = 1.0 + 0.045 * Cm        SH = 1.0 + (0.015 * Cm) * T
 *       RT = -sin((2.0 * dtheta) * rad) * RC
 *       tl = dL' / SL        tc = dC' / SC        th = dH' / SH        dE00 = sqrt(((tl * tl + tc * tc) + th * th) + (RT * tc) * th)
 *   The formula JUMPS at its branch points (P = 0, |h'_1 - h'_2| = 180, s = 360 where far): a last-place difference in atan2 there moves the result visibly.
 * MAP.  de [height][width][2] float, row 0 = bottom: (float)dEab, (float)dE00 for every pixel, labelled or not.  Optionally lab [height][width][6] float: (float)
 *   of L, a, b of A, then of B.  In the state entry pixels the context does not own read +0 in both and belong to no region.
 * PER REGION r AND METRIC k (0: ab, 1: 00), over the pixels labelled r, with v = de[p][k] (the FLOAT), six arrays [R][2]:
 *       NF = the number of pixels with v finite        NX = the number with v not finite                                              (uint64)
 *       SUM = sum (double)v        SSQ = sum (double)v * (double)v   (the product is exact)        over the pixels with v finite, binary64
 *       MAX = the largest finite v, +0 where there is none (float)        EX = the number of pixels with (double)v > t[k], strict: +inf counts, a NaN does not (uint64)
 *   The order of the binary64 additions is PROBE's and part of the definition: within a row ascending i from +0.0, one partial per row; the row partials in
 *   ascending j from +0.0; a row without a pixel of the region contributes its +0.0.
 * DERIVED BY THE HOSTS (ssh_delta_e_derive, include/ssx_host.h), each NaN where its denominator is 0:
 *       mean = SUM / NF        rms = sqrt(SSQ / NF)        max = MAX        exceed = EX / NF        coverage = NF / (NF + NX)
 * THE WHITES set the absolute size of every dE: they are a viewing decision, like exposure, and the hosts' policy (include/ssx_host.h ssh_develop_white), not
 *   this library's.  No chromatic adaptation is applied between wA and wB.
 * TWO CLASSES OF GUARANTEE.  This is the first section that uses the device library's cbrt, atan2, sin, cos, exp and sqrt in binary64:
 *   SAME BITS   the six region arrays are exactly the ordered reduction above of the map the same call returned -- a numpy walk over the returned de reproduces
 *               them bit for bit; ssx_spectral_delta_e gives the bits of ssx_delta_e_images fed with ssx_spectral_develop's two outputs (for a context that owns
 *               the whole image); several devices (each side developed by its owners, the pure entry on one) give the bits of one.
 *   WITHIN A BOUND   de and lab against the numpy restatement in binary64: the device functions are accurate to a few ulp, not correctly rounded; the bound is
 *               derived from their documented errors and the formula's partial derivatives in tests/test_delta_e_gpu.py.  Pairs within 1 degree of a branch
 *               point of dE00 are outside the bound.
 *
 * ON THE DEVICE: ssx_delta_e_rows_kernel, one workgroup per image row, takes the row in chunks of 256 pixels, one lane per pixel, writes the maps, stages the two
 * floats and the label in LDS and walks the chunk in ascending i with one lane per (quantity, metric), the accumulators in LDS indexed by the label;
 * ssx_delta_e_reduce_kernel, one lane per (quantity, r, k), walks j in ascending order (MAX takes the larger, everything else adds).  No atomics.  With the
 * feature unused nothing is allocated and nothing is launched. */

/* The colour difference as a pure function of its arguments (needs no scene): xyz_a, xyz_b [height][width][3] floats.  SUM, SSQ (binary64), MAX (float), NF, NX, EX
 * (uint64): [regions][2].  de [height][width][2], lab [height][width][6]: either may be NULL.  SSX_ERR_ARG, with ssx_last_error naming the field: a NULL required
 * pointer, an empty or too large image, regions outside 1..32 (or not 1 with labels NULL), a label that is neither a region nor 255, a white component that is not
 * finite and > 0, a threshold that is negative, infinite or NaN.  SSX_ERR_STATE: a render runs. */
int ssx_delta_e_images(ssx_ctx* ctx, uint32_t width, uint32_t height, const float* xyz_a, const float* xyz_b, const double white_a[3], const double white_b[3],
                       const uint8_t* labels /* [H][W] or NULL */, uint32_t regions, const double t[2], float* de /* [H][W][2] or NULL */, float* lab /* [H][W][6] or NULL */,
                       double* SUM, double* SSQ, float* MAX, uint64_t* NF, uint64_t* NX, uint64_t* EX /* [R][2] */);
/* Both sides developed from the context's own state by the develop kernels, weights_x [3][B] each, side x raw (denoised_x == 0) or denoised with `denoise`'s
 * parameters (the filter runs once when both sides ask for it), into device staging; then the kernels of ssx_delta_e_images on that -- the same bits.  It reads
 * only: image, sums, noise and spectral state stay as they are, so an ssx_render_continue afterwards leaves the bits of a render that was never asked.
 * SSX_ERR_STATE with ssx_spectral_develop's reasons.  SSX_ERR_ARG: what ssx_delta_e_images refuses, NULL weights, and denoised_x != 0 with denoise == NULL. */
int ssx_spectral_delta_e(ssx_ctx* ctx, const ssx_denoise_params* denoise /* or NULL */, int denoised_a, int denoised_b, const float* weights_a /* [3][B] */,
                         const float* weights_b /* [3][B] */, const double white_a[3], const double white_b[3], const uint8_t* labels /* [H][W] or NULL */, uint32_t regions,
                         const double t[2], float* de /* [H][W][2] or NULL */, float* lab /* [H][W][6] or NULL */,
                         double* SUM, double* SSQ, float* MAX, uint64_t* NF, uint64_t* NX, uint64_t* EX /* [R][2] */);

/* ---- Developing through a lens: per-bin lateral magnification and blur (appended; same ABI version) ---------------------------------------------------
 * DEVELOP is one linear map per pixel: a sensor with no optics in front of it.  This section puts a lens there, after the render: each wavelength bin is resampled
 * about the optical centre with its own magnification (lateral chromatic aberration: colour fringes at high-contrast edges) and blurred with its own separable
 * kernel (a focus that moves with wavelength, diffraction growing with lambda).  The result is again q [height][width][B], so the develop kernels, the denoiser
 * and ssx_delta_e_images take it unchanged.  The definition is this library's; a restatement in numpy gives the same bits (tests/optics_ref.py).
 *
 * All arithmetic is binary32 IEEE in the order written, every product rounded before the add, no contraction, no reassociation; non-finite values go through
 * the arithmetic as they are.  max(a, b) is a > b ? a : b and min(a, b) is a < b ? a : b (a NaN a gives b); clamp(k, lo, hi) on integers.  Input q[H][W][B]
 * row-major, row 0 = bottom, B in {4, 8, ..., 64}; pixel (i, j) has its centre at (i + 0.5, j + 0.5).  Parameters: ssx_optics_params below, R = max_radius.
 *
 * WARP.  A bin with s_b == 1.0f is copied bit for bit.  Otherwise, for pixel (i, j):
 *       dx = ((float)i + 0.5f) - cx;   x = (cx + dx * s_b) - 0.5f;   x = min(max(x, -1.0f), (float)W)
 *       i0 = floorf(x);   fx = x - i0;   ia = clamp((int)i0, 0, W-1);   ib = clamp((int)i0 + 1, 0, W-1)
 *   the same for y with j, cy, H: j0, fy, ja, jb.  Then
 *       lo = q[ja][ia][b] * (1.0f - fx) + q[ja][ib][b] * fx
 *       hi = q[jb][ia][b] * (1.0f - fx) + q[jb][ib][b] * fx
 *       w[j][i][b] = lo * (1.0f - fy) + hi * fy
 *   s_b > 1 reads further from the centre: the bin's image shrinks towards it.  The border is replicated: the field outside the render is unknown, and
 *   replicating it keeps the frame from darkening.
 * BLUR.  Separable, the horizontal pass first, then the vertical.  A bin with r_b == 0 is copied bit for bit in both passes and its taps are not read.  Otherwise
 *       acc = 0.0f;   for d = -r_b .. r_b ascending:   acc = acc + (w[j][clamp(i+d, 0, W-1)][b] * k_b[d+R])
 *   gives t[j][i][b], and the same walk over clamp(j+d, 0, H-1) on t gives out[j][i][b].  r_b may exceed the image: the clamp repeats the border.
 * THE LENS MODEL is the hosts' (libssx_host.so ssh_optics_lens, include/ssx_host.h): it makes s_b, r_b and the taps from a lateral coefficient, a blur at a
 *   reference wavelength and an axial coefficient, in binary64, rounded to binary32 once at the end.  This library takes any parameters.
 * SAME BITS: the numpy restatement; ssx_spectral_develop_optics against ssx_optics_images fed with q rebuilt from the exported sums (raw) or with
 *   ssx_denoise_spectral's output (denoised), and its `out` against ssx_develop_images of that; identity parameters (every s_b == 1, every r_b == 0) against
 *   ssx_spectral_develop.
 *
 * ON THE DEVICE (csrc/ssx_optics.hip) four kernels, none with atomics, a lane writing only its own output: ssx_optics_unpack_kernel, one wave per owned tile,
 * writes the raw source row-major; ssx_optics_warp_kernel and the two blur kernels run their lanes along the interleaved (pixel, bin) axis, so that stores and the
 * aligned part of the gathers are whole cache lines; ssx_optics_blur_h_kernel stages a row segment with its apron of R pixels either side in LDS,
 * ssx_optics_blur_v_kernel reads whole rows at the same (i, b).  A pass no bin needs (every s_b == 1; every r_b == 0) is not launched.  With the feature unused
 * nothing is allocated and nothing is launched. */
#define SSX_OPTICS_MAX_RADIUS 12u
typedef struct ssx_optics_params {
	uint32_t struct_size;      /* sizeof(ssx_optics_params) */
	float cx, cy;              /* optical centre in pixel units; finite */
	uint32_t max_radius;       /* R, 0..SSX_OPTICS_MAX_RADIUS */
	const float* scale;        /* [B]   lateral magnification s_b of bin b; finite, > 0 */
	const uint32_t* radius;    /* [B]   r_b <= R: taps visited for bin b */
	const float* taps;         /* [B][2R+1]  k_b[d+R], d = -R..R; only |d| <= r_b is read */
} ssx_optics_params;

/* WARP, then BLUR, as a pure function of its arguments (needs no scene): q [height][width][bins] -> out [height][width][bins], row-major floats.  SSX_ERR_ARG,
 * with ssx_last_error naming the field: a NULL pointer (q, out, optics, scale, radius, taps), a wrong struct_size, max_radius above 12, an r_b above max_radius, an
 * s_b that is not finite and > 0, a cx or cy that is not finite, bins not a multiple of 4 in 4..64, an empty or too large image.  SSX_ERR_STATE: a render runs. */
int ssx_optics_images(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const float* q /* [H][W][B] */, const ssx_optics_params* optics,
                      float* out /* [H][W][B] */);
/* The bins of the context's own state through the lens and then through DEVELOP, without leaving the device: the source raw (denoise == NULL) or denoised, as in
 * ssx_spectral_develop; WARP and BLUR on it; then the develop kernels with weights [channels][B] on the result.  bins_out [H][W][B]: the bins behind the lens;
 * out [H][W][channels]: their development; either may be NULL (both NULL: the kernels run and the results stay on the device -- for measurements), and with
 * out == NULL the weights may be NULL too: nothing is developed.  It reads only: image, sums, noise and spectral state stay as they are, so an ssx_render_continue
 * afterwards leaves the bits of a one-shot render in the image and in ssx_spectral_read.  SSX_ERR_STATE with ssx_spectral_develop's reasons, and where the context
 * does not own every tile (tile_stride != 1): a blur needs its neighbours.  SSX_ERR_ARG: what ssx_optics_images and ssx_spectral_develop refuse. */
int ssx_spectral_develop_optics(ssx_ctx* ctx, const ssx_denoise_params* denoise /* or NULL */, const ssx_optics_params* optics, const float* weights /* [C][B] */,
                                uint32_t channels, float* out /* [H][W][C] or NULL */, float* bins_out /* [H][W][B] or NULL */);

/* ---- Depth of field after the render: per-bin defocus from the depth guide (appended; same ABI version) -------------------------------------------------
 * The lens above has no aperture: its blur is the same everywhere in the frame.  This section gives it one, still after the render (the camera of the path
 * kernels is a pinhole and stays one): every (pixel, bin) is spread over a disc whose radius -- the circle of confusion -- grows with the distance, in inverse
 * depth, between the pixel's surface (the depth guide of ssx_guides) and the bin's focus.  A focus that moves with the wavelength is longitudinal chromatic
 * aberration: surfaces in front of and behind the focus fringe in different colours.  The result is again q [height][width][B].  The definition is this
 * library's; a restatement in numpy gives the same bits (tests/defocus_ref.py).
 *
 * All arithmetic is binary32 IEEE in the order written, every product rounded before the add, no contraction, no reassociation; min and max as above
 * (a NaN first argument gives the second); sqrtf and / are correctly rounded; non-finite values go through the arithmetic as they are.  Input q[H][W][B]
 * row-major, row 0 = bottom, B in {4, 8, ..., 64}; depth[H][W]; parameters: ssx_defocus_params below, R = max_radius, K = gain, f_b = focus[b].
 *
 * DEFOCUS.  Per pixel s:
 *       inv[s] = depth[s] > 0.0f ? 1.0f / depth[s] : 0.0f
 *   a miss (depth 0), a NaN, a negative depth and +inf are all "infinitely far".  Per pixel s and bin b:
 *       c[s][b] = min(fabsf(inv[s] - f_b) * K, (float)R)                          the circle of confusion, in pixels
 *       a[s][b] = 1.0f / (3.14159274f * ((c * c + c) + 0.333333343f))             c = c[s][b]
 *   the divisor is the integral over the plane of the cover function below (a disc of radius c with a linear skirt one pixel wide): a wide disc is
 *   correspondingly faint.  Per destination pixel p = (i, j) and bin b:
 *       sw = 0.0f;   sq = 0.0f
 *       for dy = -R .. R ascending, and inside it for dx = -R .. R ascending:   s = (i + dx, j + dy), skipped where it lies outside the image
 *           ce = inv[s] < inv[p] ? min(c[s][b], c[p][b]) : c[s][b]
 *           dist = sqrtf((float)(dx * dx + dy * dy));   cover = min(max((ce + 1.0f) - dist, 0.0f), 1.0f)
 *           taken only if cover > 0.0f:   w = cover * a[s][b];   sw = sw + w;   sq = sq + w * q[s][b]
 *       out[p][b] = sq / sw
 *   The border is NOT replicated: the sum is normalised, so the frame does not darken.  ce: a source behind the destination cannot spread over it further than
 *   the destination's own blur, so a sharp foreground stays clean against a blurred background (and a blurred foreground still spreads over a sharp
 *   background).  A non-finite q outside its own disc poisons nothing: its tap is not taken.  The centre tap always counts (cover == 1, a > 0): sw > 0.
 *   With K == 0 or R == 0 the stage is a bit-for-bit copy and nothing is launched.  ELSEWHERE AN IN-FOCUS PIXEL IS NOT COPIED: a pixel that only its own tap
 *   reaches comes out as (a * q) / a with a = a[p][b] -- two roundings from q, not q.
 * THE THIN LENS is the hosts' (libssx_host.so ssh_defocus_thin_lens, include/ssx_host.h): K and f_b from an aperture, a focus distance and an axial
 *   coefficient.  The guide's depth is a RAY LENGTH from the eye, not a distance along the optical axis: the surface in focus is a sphere about the eye.
 * SAME BITS: the numpy restatement; ssx_spectral_develop_lens against ssx_defocus_images (q rebuilt from the exported sums or ssx_denoise_spectral's output,
 *   depth from ssx_guides), ssx_optics_images and ssx_develop_images in a chain; defocus == NULL against ssx_spectral_develop_optics; both NULL against
 *   ssx_spectral_develop.
 *
 * ON THE DEVICE (csrc/ssx_defocus.hip) two kernels, neither with atomics, a lane writing only its own output: ssx_defocus_prepare_kernel writes inv[H][W] and
 * a[H][W][B] (c is three operations on inv and f_b, and the gather redoes them in registers, to the same bits, instead of reading a third array);
 * ssx_defocus_gather_kernel stages a tile of 16 x 16 pixels with its apron of R pixels, four bins at a time, in LDS and walks (dy, dx) uniformly across the wave.
 * With the feature unused nothing is allocated and nothing is launched. */
#define SSX_DEFOCUS_MAX_RADIUS 12u
typedef struct ssx_defocus_params {
	uint32_t struct_size;      /* sizeof(ssx_defocus_params) */
	uint32_t max_radius;       /* R, 0..SSX_DEFOCUS_MAX_RADIUS: the largest circle of confusion, in pixels */
	float gain;                /* K: pixels of blur radius per unit of inverse-depth offset; finite, >= 0 */
	const float* focus;        /* [B]   f_b: the inverse focus distance of bin b; finite, >= 0 (0: focused at infinity) */
} ssx_defocus_params;

/* DEFOCUS as a pure function of its arguments (needs no scene): q [height][width][bins], depth [height][width] -> out [height][width][bins], row-major floats.
 * SSX_ERR_ARG, with ssx_last_error naming the field: a NULL pointer (q, depth, out, defocus, focus), a wrong struct_size, max_radius above 12, a gain or a
 * focus[b] that is not finite or is negative, bins not a multiple of 4 in 4..64, an empty or too large image.  SSX_ERR_STATE: a render runs. */
int ssx_defocus_images(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const float* q /* [H][W][B] */, const float* depth /* [H][W] */,
                       const ssx_defocus_params* defocus, float* out /* [H][W][B] */);
/* ssx_spectral_develop_optics with an aperture: the source as there (raw through the same unpack kernel, or denoised); DEFOCUS on it with the context's own
 * guide depth (the guides are computed if they are not yet held); then WARP and BLUR; then the develop kernels.  DEFOCUS comes first because the depth map is
 * registered to the unwarped pixels.  defocus NULL: no DEFOCUS -- the bits of ssx_spectral_develop_optics; optics NULL: no WARP or BLUR; both NULL: the bits of
 * ssx_spectral_develop.  out, bins_out and weights as in ssx_spectral_develop_optics.  It reads only.  SSX_ERR_STATE with ssx_spectral_develop_optics's
 * reasons, tile_stride != 1 among them (whatever is NULL); SSX_ERR_ARG: what ssx_defocus_images, ssx_optics_images and ssx_spectral_develop refuse. */
int ssx_spectral_develop_lens(ssx_ctx* ctx, const ssx_denoise_params* denoise /* or NULL */, const ssx_defocus_params* defocus /* or NULL */,
                              const ssx_optics_params* optics /* or NULL */, const float* weights /* [C][B] */, uint32_t channels,
                              float* out /* [H][W][C] or NULL */, float* bins_out /* [H][W][B] or NULL */);

/* ---- Developing onto a sensor: colour filter array, noise, ADC and demosaic (appended; same ABI version) ------------------------------------------------
 * DEVELOP evaluates complete response curves at every pixel, without noise and without quantisation.  A camera's sensor does none of that: each photosite sits
 * behind ONE filter of a colour filter array, counts electrons (shot noise, read noise), the count goes through an ADC, and the three colours are then
 * interpolated from one channel per pixel -- which is where zipper and false-colour artefacts come from.  A photosite integrates the spectrum under its own
 * filter, and the bins hold exactly that: a mosaic taken from the bins is right, one taken from a developed RGB image is not.  Two stages, SENSOR and
 * DEMOSAIC; the definition is this library's; a restatement in numpy gives the same bits (tests/sensor_ref.py).
 *
 * All arithmetic is binary32 IEEE in the order written, every product rounded before the add, no contraction, no reassociation; max(a, b) is a > b ? a : b and
 * min(a, b) is a < b ? a : b (a NaN a gives b); sqrtf and / are correctly rounded, floorf is exact; non-finite values go through the arithmetic as they are.
 * Images are row-major, row 0 = bottom; B in {4, 8, ..., 64}; W >= 3 and H >= 3.  Parameters: ssx_sensor_params below.
 *
 * SENSOR.  q[H][W][B] -> raw[H][W] (and dn[H][W] with an ADC).  For pixel (i, j), p = j * W + i (uint32):
 *       c = cfa[(j & 1) * 2 + (i & 1)]                                            the photosite's filter, 0..2
 *       v = 0.0f;   for b = 0 .. B-1 ascending:   v = v + (q[j][i][b] * weights[c][b])          DEVELOP's accumulation for that one channel
 *       e = v * exposure                                                          electrons
 *   only with noise != 0:
 *       sd = sqrtf(max(e, 0.0f) + read_var);   e = e + sd * z(p)
 *   only with white > 0.0f (an ADC):
 *       d = floorf((e * dn_per_e + black) + 0.5f);   d = min(max(d, 0.0f), white);   dn[j][i] = d;   e = (d - black) * e_per_dn
 *   then
 *       raw[j][i] = e * inv_exposure                                              back in the units of q * weights: comparable with a plain develop
 *   z(p) is a stateless standard normal made of integers only, so that every implementation gives the same bits.  On uint32, wrapping:
 *       h(x):   x ^= x >> 16;   x *= 0x7feb352d;   x ^= x >> 15;   x *= 0x846ca68b;   x ^= x >> 16
 *       u_k = h(h(h(h(seed) + frame) + p) + k)   for k = 0 .. 5;      S = the integer sum of the twelve 16-bit halves of u_0 .. u_5
 *       z = ((float)S - 393210.0f) * 1.52587890625e-05f
 *   the classic sum of twelve uniforms: both operations are exact, the mean is 0, the variance 1 - 2^-32, the tails end at +-6.  THE SHOT NOISE IS THEREFORE
 *   GAUSSIAN WITH THE POISSON VARIANCE: that is wrong below a few electrons (a count is a non-negative integer and its distribution is skewed; here e may go
 *   negative before the ADC clamps it), and exact Poisson counts are out of scope.  A NaN e takes sd = sqrtf(read_var) and stays NaN; with an ADC a NaN d
 *   becomes 0.  Fixed-pattern noise, dark current, blooming and cross-talk are out of scope.
 * DEMOSAIC.  raw[H][W] -> out[H][W][3], with any tables taps[4][3][25] -- indexed by phase, output channel and (dy + 2) * 5 + (dx + 2) -- and ccm[3][3].
 *   m(k, n) = k < 0 ? -k : (k >= n ? 2 * (n - 1) - k : k): the border is mirrored about the edge pixel without repeating it, which keeps the parity of the
 *   colour filter array (a clamp would break it).  For pixel (i, j), phase = (j & 1) * 2 + (i & 1), for c = 0 .. 2:
 *       acc = 0.0f;   for dy = -2 .. 2 ascending, and inside it for dx = -2 .. 2 ascending:
 *           acc = acc + (raw[m(j + dy, H)][m(i + dx, W)] * taps[phase][c][(dy + 2) * 5 + (dx + 2)])           every tap is visited, zero coefficients included
 *       rgb[c] = acc
 *   and for c' = 0 .. 2:   out[j][i][c'] = ((0.0f + rgb[0] * ccm[c'][0]) + rgb[1] * ccm[c'][1]) + rgb[2] * ccm[c'][2]
 *   (a zero coefficient on a non-finite raw gives NaN, as the arithmetic says; -0 through an identity ccm comes out as +0).
 * THE TABLES are the hosts' (libssx_host.so, include/ssx_host.h): ssh_sensor_bayer makes cfa and taps for the four Bayer patterns, bilinear or
 *   Malvar-He-Cutler; ssh_sensor_exposure the electron and ADC scales; ssh_sensor_ccm the least-squares matrix.  This library takes any tables.
 * SAME BITS: the numpy restatement; SENSOR with noise off, no ADC and exposure == inv_exposure == 1 against ssx_develop_images at [j][i][cfa]; DEMOSAIC with
 *   identity taps and an identity ccm against raw (up to -0); ssx_spectral_develop_sensor against ssx_defocus_images, ssx_optics_images, ssx_sensor_images
 *   and ssx_demosaic_images in a chain.
 *
 * ON THE DEVICE (csrc/ssx_sensor.hip) two kernels, neither with atomics, a lane writing only its own output: ssx_sensor_kernel, one lane per pixel, reads q
 * once with the weights at wave-uniform addresses (all three channels accumulated, the photosite's selected); ssx_demosaic_kernel, one lane per 2 x 2 quad,
 * stages a tile of 64 x 16 pixels with its apron of 2 in LDS, mirroring while it stages, with all four phases' tables at wave-uniform addresses.  With the
 * feature unused nothing is allocated and nothing is launched. */
typedef struct ssx_sensor_params {
	uint32_t struct_size;      /* sizeof(ssx_sensor_params) */
	uint32_t cfa[4];           /* the filter (0..2: the row of `weights`, the channel of `taps`) at phase (j & 1) * 2 + (i & 1); row 0 = bottom */
	uint32_t noise;            /* 0: no noise */
	uint32_t seed, frame;      /* of z(p): another frame of the same seed is an independent exposure */
	float exposure;            /* electrons per unit of q * weights; finite, >= 0 */
	float inv_exposure;        /* finite; the hosts pass 1 / exposure */
	float read_var;            /* the read noise's variance in electrons^2; finite, >= 0 */
	float dn_per_e, e_per_dn;  /* the ADC's gain and its inverse; finite */
	float black, white;        /* the ADC's offset and its largest number, in DN; finite, white >= 0, white == 0: no ADC; black <= white with an ADC */
	const float* weights;      /* [3][B]     SENSOR: the three filters' response per bin (ssh_develop_weights with a camera's curves) */
	const float* taps;         /* [4][3][25] DEMOSAIC; finite */
	const float* ccm;          /* [3][3]     DEMOSAIC; finite */
} ssx_sensor_params;

/* SENSOR as a pure function of its arguments (needs no scene): q [height][width][bins] -> raw [height][width], dn [height][width] or NULL (dn needs an ADC).
 * taps and ccm are not read.  SSX_ERR_ARG, with ssx_last_error naming the field: a NULL pointer (q, raw, sensor, weights), a wrong struct_size, a cfa entry
 * above 2, an exposure, inv_exposure, read_var, dn_per_e, e_per_dn, black or white that is not finite, a negative exposure, read_var or white, black > white
 * with white > 0, dn without an ADC, bins not a multiple of 4 in 4..64, width or height below 3, a too large image.  SSX_ERR_STATE: a render runs. */
int ssx_sensor_images(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const float* q /* [H][W][B] */, const ssx_sensor_params* sensor,
                      float* raw /* [H][W] */, float* dn /* [H][W] or NULL */);
/* DEMOSAIC as a pure function of its arguments: raw [height][width] -> out [height][width][3].  weights is not read.  SSX_ERR_ARG: a NULL pointer (raw, out,
 * sensor, taps, ccm), a tap or a ccm entry that is not finite, and what ssx_sensor_images refuses in the struct and the size.  SSX_ERR_STATE: a render runs. */
int ssx_demosaic_images(ssx_ctx* ctx, uint32_t width, uint32_t height, const float* raw /* [H][W] */, const ssx_sensor_params* sensor, float* out /* [H][W][3] */);
/* ssx_spectral_develop_lens onto a sensor: the source and the stages of ssx_spectral_develop_lens (raw or denoised; DEFOCUS; WARP and BLUR; either may be
 * NULL), then SENSOR instead of the develop kernels, then DEMOSAIC; nothing leaves the device in between.  out [H][W][3], raw_out [H][W], dn_out [H][W]
 * (needs an ADC): any may be NULL.  It reads only, as ssx_spectral_develop_optics does.  SSX_ERR_STATE with ssx_spectral_develop_lens's reasons, tile_stride != 1
 * among them; SSX_ERR_ARG: what ssx_defocus_images, ssx_optics_images, ssx_sensor_images and ssx_demosaic_images refuse. */
int ssx_spectral_develop_sensor(ssx_ctx* ctx, const ssx_denoise_params* denoise /* or NULL */, const ssx_defocus_params* defocus /* or NULL */,
                                const ssx_optics_params* optics /* or NULL */, const ssx_sensor_params* sensor, float* out /* [H][W][3] or NULL */,
                                float* raw_out /* [H][W] or NULL */, float* dn_out /* [H][W] or NULL */);

/* ---- Glare: per-bin convolution by FFT ------------------------------------------------------------
 * Veiling glare, diffraction rings and spikes: wide, non-separable, wavelength-dependent point spread functions that neither BLUR (separable, radius 12) nor
 * DEFOCUS (a gather, (2 R + 1)^2 taps) can reach.  Per wavelength bin the image is padded, transformed, multiplied by the psf's transform, transformed back
 * and cropped.  The conventions are those of "Developing through a lens": binary32 IEEE in the order written, every product rounded before the add, no
 * contraction, no reassociation.  Input q[H][W][B], row 0 at the bottom, B in {4, 8, ..., 64}.  The library takes any tables; the host policy that makes an
 * aperture's is ssh_glare_aperture (include/ssx_host.h).
 *
 * TWIDDLES are the caller's (ssh_glare_twiddles): no sine or cosine of the device or of a libm enters the bits.
 *
 * FFT(x[0..P), T, inverse) on complex binary32 values is defined by its butterfly graph.  n = log2 P.
 *   y[k] = x[bitrev_n(k)]
 *   for s = 1..n, h = 2^(s-1), step = P / (2 h), every block base g = 0, 2h, 4h, ... and every k in 0..h-1:
 *     w = T[k * step]                           (inverse: w.im = -w.im)
 *     a = y[g+k];  b = y[g+k+h]
 *     t.re = (w.re * b.re) - (w.im * b.im)
 *     t.im = (w.re * b.im) + (w.im * b.re)
 *     y[g+k]   = (a.re + t.re, a.im + t.im)
 *     y[g+k+h] = (a.re - t.re, a.im - t.im)
 * The product with T[0] is performed like any other: the table need not hold (1, 0).  Any schedule that executes this graph gives these bits.
 *
 * GLARE, per bin b with on[b] != 0 (a bin with on[b] == 0 is copied bit for bit and its psf is not read):
 *   PAD       X[jj][ii], jj < py, ii < px.  i' = ii < W + R ? ii : ii - px, j' likewise with H and py.  Where -R <= i' < W + R and -R <= j' < H + R:
 *             X = (q[clamp(j', 0, H-1)][clamp(i', 0, W-1)][b], 0), elsewhere (0, 0).  The border is replicated, so the frame does not darken; px >= W + 2 R, so
 *             the two aprons never meet.
 *   KERNEL    Kp = 0, then Kp[dy mod py][dx mod px] = (psf_b[dy+R][dx+R], 0) for |dy|, |dx| <= R.
 *   FORWARD   of both: every row with twiddle_x, then every column with twiddle_y.
 *   MULTIPLY  Y = X (x) Kf, the complex product written as t above.
 *   INVERSE   every column, then every row, with the conjugated twiddles.
 *   CROP      out[j][i][b] = Y[j][i].re * inv, inv = 1 / (px py), which is exact.  The imaginary part is dropped.
 * That is out(j, i) = sum psf(dy, dx) q(j - dy, i - dx): a convolution, not a correlation.
 * The result is not clamped: where the true value is ~0 it may come out slightly negative.  A non-finite value anywhere in a bin makes that whole bin's output
 * non-finite; other bins are not touched.  With every on[b] == 0 nothing is allocated or launched and out is a copy.
 * Scratch on the device: 16 px py bytes per bin in flight; bins are processed in chunks of whole groups of four that fit 256 MiB, at least one group
 * (64 px py bytes: 1 GiB at the largest plan, at most 256 MiB wherever px py <= 2^22); beside these planes the context keeps the packed twiddles
 * (16 (px + py) bytes), the psf (4 B (2R+1)^2 bytes: 67 MB at B = 64, R = 256), out (4 B W H bytes) and, for ssx_glare_images, q (4 B W H bytes), all of it
 * from the first glare until ssx_destroy. */
#define SSX_GLARE_MAX_RADIUS 256u
#define SSX_GLARE_MAX_EXTENT 4096u
typedef struct ssx_glare_params {
	uint32_t struct_size;
	uint32_t radius;           /* R, 0..SSX_GLARE_MAX_RADIUS; K = 2R+1 */
	uint32_t px, py;           /* padded extents: the smallest powers of two >= max(2, W+2R) and max(2, H+2R); <= SSX_GLARE_MAX_EXTENT (ssh_glare_plan) */
	const uint8_t* on;         /* [B]  0: the bin is copied bit for bit, its psf is not read */
	const float* psf;          /* [B][K][K]  psf_b[dy+R][dx+R]; finite */
	const float* twiddle_x;    /* [px/2][2]  (re, im) of the forward twiddle T[m]; finite */
	const float* twiddle_y;    /* [py/2][2] */
} ssx_glare_params;

/* GLARE as a pure function of its arguments (needs no scene): q [height][width][bins] -> out [height][width][bins].  SSX_ERR_ARG, with ssx_last_error naming the
 * field: bins not a multiple of 4 in 4..64, a NULL pointer (q, out, glare, on, psf, twiddle_x, twiddle_y), an empty or too large image, a wrong struct_size, a
 * radius above SSX_GLARE_MAX_RADIUS, px or py not the defined value or above SSX_GLARE_MAX_EXTENT, a psf entry of an `on` bin or (with some bin on) a twiddle
 * entry that is not finite.  SSX_ERR_STATE: a render runs. */
int ssx_glare_images(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const float* q /* [H][W][B] */, const ssx_glare_params* glare, float* out /* [H][W][B] */);
/* ssx_spectral_develop_lens with GLARE between the lens and the develop kernels: the source and the stages of ssx_spectral_develop_lens (raw or denoised;
 * DEFOCUS; WARP and BLUR; either may be NULL), then GLARE, then the develop kernels; nothing leaves the device in between.  glare == NULL gives the bits of
 * ssx_spectral_develop_lens.  out, weights and bins_out as there; bins_out holds the bins behind the glare.  It reads only.  Glare in front of a sensor goes
 * by way of bins_out and ssx_sensor_images / ssx_demosaic_images.  SSX_ERR_STATE with ssx_spectral_develop_lens's reasons, tile_stride != 1 among them;
 * SSX_ERR_ARG: what ssx_spectral_develop_lens and ssx_glare_images refuse. */
int ssx_spectral_develop_glare(ssx_ctx* ctx, const ssx_denoise_params* denoise /* or NULL */, const ssx_defocus_params* defocus /* or NULL */,
                               const ssx_optics_params* optics /* or NULL */, const ssx_glare_params* glare /* or NULL */, const float* weights /* [C][B] */,
                               uint32_t channels, float* out /* [H][W][C] or NULL */, float* bins_out /* [H][W][B] or NULL */);

/* ---- Finishing a development for a display: meter, local tone map, tone curve (appended; same ABI version) ----------------------------------------
 * A development is a linear image with the dynamic range of the scene: a light hundreds of times brighter than the walls it lights, and the glare around it.  A
 * display takes [0, 1] through a transfer function.  Three stages take one to the other: METER counts what the image holds, LOCAL compresses its large-scale
 * contrast and keeps the detail, TONE applies channel gains, a matrix and a curve.  What to aim for -- the exposure, the white point, the curve -- is the hosts'
 * policy (include/ssx_host.h: ssh_meter_derive, ssh_tone_curve, ssh_display_matrix); this library takes any numbers.  NO log, exp OR pow RUNS ON THE DEVICE: the
 * logarithm is the integer one a binary32's bit pattern already is, the curve with the display's transfer function is the caller's table, counts are integers.
 * So every output has the bits of a restatement in numpy (tests/display_ref.py), not "within a bound".
 *
 * Binary32 IEEE in the order written, every product rounded before the add, no contraction, no reassociation; max(a, b) is a > b ? a : b and min(a, b) is
 * a < b ? a : b (a NaN a gives b); / is correctly rounded, floorf is exact; bits(x) is x's pattern as uint32, frombits its inverse.  Images are row-major, row
 * 0 = bottom.  Luminance of a pixel x[3]:   y = ((0.0f + x[0] * luma[0]) + x[1] * luma[1]) + x[2] * luma[2];   luma[3] finite.
 *
 * METER.  img[H][W][3], luma, mask (uint8 [H][W] or NULL; 0 = the pixel is not counted) -> hist uint32 [4][SSX_METER_KEYS], special uint32 [4][4].  The
 *   quantities are k = 0 .. 2, the channels, and k = 3, y.  For a counted pixel's value x with u = bits(x):
 *       x == +-0 -> special[k][0];   a NaN -> special[k][3];   else negative (-inf too) -> special[k][1];   +inf -> special[k][2];   else hist[k][u >> 19] += 1
 *   sixteen keys per octave (the exponent and the top four bits of the significand), subnormals in keys 0 .. 15; keys 4080 and above stay 0.  Key K's lower edge
 *   is frombits(K << 19).  Counts are integers (modulo 2^32: an image has at most 2^28 pixels), so any order of addition gives these numbers.
 * LOCAL.  img, luma, ssx_local_params -> gain[H][W] and, where asked for, base[H][W].  Per pixel
 *       yc = min(max(y * exposure, y_lo), y_hi)                                     a NaN gives y_lo; y_lo <= y_hi are positive, normal and finite
 *       L  = (float)((int32)(bits(yc) >> 7) - 8323072) * 0x1p-16f                  the piecewise-linear log2: exponent - 127 + the top 16 bits of the fraction; exact
 *   then the self-guided filter of He, Sun and Tang ("Guided image filtering", ECCV 2010) on L, radius r = 1 .. SSX_LOCAL_MAX_RADIUS, n = (float)((2r+1) * (2r+1)),
 *   the window's coordinates clamped to the image (the count stays n), c(k, n) = min(max(k, 0), n - 1):
 *       box(P)[j][i]:   h[j][i] = 0.0f, then for dx = -r .. r ascending   h = h + P[j][c(i + dx, W)];      s[j][i] = 0.0f, then for dy = -r .. r ascending   s = s + h[c(j + dy, H)][i]
 *       S1 = box(L);   S2 = box(LL), LL[j][i] = (L * L) rounded
 *       m = S1 / n;   v = max(S2 / n - (m * m), 0.0f);   a = v / (v + eps);   b = m - (a * m)                 eps finite and positive
 *       A = box(a) / n;   Bm = box(b) / n;   base = (A * L) + Bm
 *   and the compression about a pivot, with detail kept:
 *       t = ((base - pivot) * compress) + pivot;   Lo = t + ((L - base) * boost);   gain = E(Lo - L)
 *       E(d):   f = floorf(d * 65536.0f);   f = min(max(f, -16777216.0f), 16777216.0f)  (a NaN gives the lower bound);   frombits(min(max((int32)f + 8323072, 0x10000), 0xFEFFFF) << 7)
 *   E is L's inverse: E(L(y)) is y with its low 7 bits cleared, and a gain is always a positive normal number.  The clamp in binary32 in front of the conversion is
 *   there because an int32 conversion of a NaN or of 2^31 is nobody's definition; pivot, compress and boost need only be finite.  compress = boost = 1 gives gain = 1.
 * TONE.  img, local[H][W] or NULL, ssx_tone_params -> out[H][W][3].  Per pixel, for c = 0 .. 2:   v[c] = img[c] * gains[c];   with local:   v[c] = v[c] * local[j][i];
 *       x[c'] = ((0.0f + v[0] * matrix[c'][0]) + v[1] * matrix[c'][1]) + v[2] * matrix[c'][2]
 *       xc = min(max(x, lo), hi);   k = bits(xc) - bits(lo);   idx = k >> shift;   f = (float)(k & ((1u << shift) - 1u)) * 2^-shift          (exact)
 *       out = curve[idx] + ((curve[idx + 1] - curve[idx]) * f)
 *   The table has curve_len = ((bits(hi) - bits(lo)) >> shift) + 2 entries, at most SSX_TONE_MAX_CURVE; shift is 12 .. 23; lo <= hi are positive, normal and finite.
 *   Node idx stands at frombits(bits(lo) + (idx << shift)): 2^(23 - shift) nodes per octave, interpolated linearly in the bit pattern (so linearly in x within an
 *   octave).  A NaN, a negative value and -0 are taken at lo.  The table holds the tone curve and the display's transfer function composed (ssh_tone_curve); this
 *   library takes any finite table, and does not clamp the result.
 * SAME BITS: the numpy restatement, on every case of tests/display_cases.py (a zero may differ in sign where the arithmetic leaves that open to -0 + 0 orders:
 *   none is known).  ssx_meter_images's counts are equal as integers.
 *
 * ON THE DEVICE (csrc/ssx_display.hip): ssx_meter_kernel keeps one quantity's 4096 + 4 counters in LDS per workgroup (16 KB: eight workgroups per CU), adds with
 * integer LDS atomics -- equal keys of a wave are counted first and added once, two rounds, the rest lane by lane -- and flushes its non-zero counters with integer
 * global atomics.  LOCAL is four launches of two kernels, rows then columns, twice, each staging its window through LDS with both planes in one pass; m, v, a, b
 * end the first column pass, base, Lo and the gain the second.  ssx_tone_kernel is one lane per pixel with the table read through the caches.  A lane writes only
 * its own output; no float atomics.  With the feature unused nothing is allocated and nothing is launched. */
#define SSX_METER_KEYS 4096u
#define SSX_LOCAL_MAX_RADIUS 32u
#define SSX_TONE_MAX_CURVE 16384u
typedef struct ssx_local_params {
	uint32_t struct_size;      /* sizeof(ssx_local_params) */
	uint32_t radius;           /* r, 1..SSX_LOCAL_MAX_RADIUS */
	float exposure;            /* finite */
	float y_lo, y_hi;          /* positive, normal, finite, y_lo <= y_hi */
	float eps;                 /* finite, > 0: the variance of L (octaves squared) below which a window counts as flat */
	float pivot;               /* finite: the L that keeps its place (the hosts pass L of the key value) */
	float compress, boost;     /* finite: the factor on the base layer's distance from the pivot, and on the detail */
} ssx_local_params;
typedef struct ssx_tone_params {
	uint32_t struct_size;      /* sizeof(ssx_tone_params) */
	uint32_t shift;            /* 12..23 */
	uint32_t curve_len;        /* ((bits(hi) - bits(lo)) >> shift) + 2, at most SSX_TONE_MAX_CURVE */
	float lo, hi;              /* positive, normal, finite, lo <= hi */
	float gains[3];            /* finite */
	float matrix[9];           /* [c'][c], finite */
	const float* curve;        /* [curve_len], finite */
} ssx_tone_params;

/* METER as a pure function of its arguments (needs no scene): img [height][width][3], luma [3], mask [height][width] or NULL -> hist [4][SSX_METER_KEYS],
 * special [4][4].  SSX_ERR_ARG, with ssx_last_error naming the field: a NULL pointer (img, luma, hist, special), a luma entry that is not finite, an empty or too
 * large image.  SSX_ERR_STATE: a render runs. */
int ssx_meter_images(ssx_ctx* ctx, uint32_t width, uint32_t height, const float* img /* [H][W][3] */, const float* luma /* [3] */, const uint8_t* mask /* [H][W] or NULL */,
                     uint32_t* hist /* [4][4096] */, uint32_t* special /* [4][4] */);
/* LOCAL as a pure function of its arguments: img [height][width][3], luma [3] -> gain [height][width], base [height][width] or NULL.  SSX_ERR_ARG: a NULL pointer
 * (img, luma, local, gain), a wrong struct_size, a radius outside 1..SSX_LOCAL_MAX_RADIUS, an exposure, pivot, compress or boost that is not finite, a y_lo or
 * y_hi that is not a positive normal number, y_lo > y_hi, an eps that is not finite and positive, a luma entry that is not finite, an empty or too large image.
 * SSX_ERR_STATE: a render runs. */
int ssx_local_images(ssx_ctx* ctx, uint32_t width, uint32_t height, const float* img /* [H][W][3] */, const float* luma /* [3] */, const ssx_local_params* local,
                     float* gain /* [H][W] */, float* base /* [H][W] or NULL */);
/* TONE as a pure function of its arguments: img [height][width][3], local [height][width] or NULL -> out [height][width][3].  SSX_ERR_ARG: a NULL pointer (img,
 * tone, curve, out), a wrong struct_size, a shift outside 12..23, a lo or hi that is not a positive normal number, lo > hi, a curve_len that is not the defined
 * value or above SSX_TONE_MAX_CURVE, a gains, matrix or curve entry that is not finite, an empty or too large image.  SSX_ERR_STATE: a render runs. */
int ssx_tone_images(ssx_ctx* ctx, uint32_t width, uint32_t height, const float* img /* [H][W][3] */, const float* local /* [H][W] or NULL */, const ssx_tone_params* tone,
                    float* out /* [H][W][3] */);

/* ---- Diagnostics for the parity tests (not part of the reference's interface) ---------------------
 * ssx_debug_eval runs one building block of the path kernel -- the same device function the kernel
 * inlines -- on n items, one per lane: `in` holds in_words 32-bit words per item, `out` receives
 * out_words (<= 12) per item.  A scene must be uploaded (its tables are staged as in a render). */
enum {
	SSX_DBG_FMATH = 1,        /* in: x                                  out: sin, cos, acos, sincos.s, sincos.c (include/ssx_fmath.h) */
	SSX_DBG_SPHTRI = 2,       /* in: A[3], B[3], C[3]                   out: b, cos_c, alpha, cos_alpha, area (src/util/spherical-tri.cpp:18-124) */
	SSX_DBG_ARVO = 3,         /* in: A, B, C, b, cos_c, alpha, cos_alpha, area, rng[4]   out: dir[3], rng state lo, hi (src/util/random.cpp:101-154) */
	SSX_DBG_SAMPLE_LIGHT = 4, /* in: from[3], rng[4]                    out: dir[3], light quad, pdf, rng state lo, hi (src/scene.cpp:417-431) */
	SSX_DBG_COSHEMI = 5,      /* in: normal[3], rng[4]                  out: w_i[3], pdf, rng state lo, hi (src/util/random.cpp:29-49 + math-helpers.hpp:35-39) */
	SSX_DBG_TRACE = 6,        /* in: orig[3], dir[3], ignore quad (int) out: quad (0xFFFFFFFF: none), triangle of the quad, dist, st[2] (src/scene.cpp:433-445) */
	SSX_DBG_RAND_CHOICE = 7,  /* in: rng[4], n                          out: choice, rng state lo, hi (src/util/random.hpp:75-78) */
	SSX_DBG_ALBEDO = 8,       /* in: quad, st[2], lambda_0              out: albedo[4] (src/material.cpp:45-143) */
	SSX_DBG_FLUX_TO_XYZ = 9,  /* in: flux[4], lambda_0                  out: X, Y, Z (src/util/color.hpp:115-139) */
	SSX_DBG_RAND_1F = 10,     /* in: rng[4]                             out: rand_1f, rng state lo, hi (src/util/random.hpp:68-70) */
	/* libm = glibc-2.35 (ssx_render_params.libm): the units the _glibc kernels inline, same inputs and outputs as the op above them */
	SSX_DBG_GLIBC_MATH = 11,  /* in: x                                  out: sinf, cosf, acosf, sincosf.s, sincosf.c (include/ssx_glibc_math.h) */
	SSX_DBG_SPHTRI_GLIBC = 12, SSX_DBG_ARVO_GLIBC = 13, SSX_DBG_SAMPLE_LIGHT_GLIBC = 14, SSX_DBG_COSHEMI_GLIBC = 15,
	/* SSX_DBG_TRACE restricted to a set of primitives, as ssx_generate_kernel traces a tile's camera rays (default libm's kernel).  mask[4]: bit q & 31 of word
	 * q >> 5 = primitive q may be hit; a primitive whose bit is clear is left out.  The device function reads the mask ONCE PER WAVE (through the first lane:
	 * in a render it is the tile's), so the items are taken in blocks of 64 -- items 64 b .. 64 b + 63 -- and every item of a block must carry the same four
	 * words: the caller pads its last block, e.g. with copies of its final row.  Bits at or above the number of primitives are ignored. */
	SSX_DBG_TRACE_MASKED = 16, /* in: orig[3], dir[3], ignore quad (int), mask[4]   out: as SSX_DBG_TRACE */
	/* The trace the context's renders run for bounce and shadow rays.  SSX_DBG_TRACE and SSX_DBG_TRACE_MASKED run the generic loop whatever the scene; this op
	 * runs the body specialised to the context's mesh topology (ssx_kernel_variant(): 1 Cornell, 2 plane, 3 the scene's own pattern, e.g. after
	 * ssx_set_jit(ctx, SSX_JIT_AT_UPLOAD)): its generated pass 1, and the pass 2 that finds a candidate's vertices in the distinct-vertex table.  Same upload,
	 * same rows, same answers as SSX_DBG_TRACE is the contract the tests hold it to.  has_ray = 0: the lane takes part in the wave's pass 1 and traces
	 * nothing, as an idle lane of a shadow-ray flush; its answer is "none", distance +inf, st 0.  SSX_ERR_STATE on a context that runs the generic kernel
	 * (topology 0; the op would be SSX_DBG_TRACE), and where the debug kernel of a scene's own pattern cannot be compiled: that kernel lives in a debug-only
	 * variant of the pattern's run-time program, compiled (or loaded from the disk cache) at the first call; the production variants are untouched by it. */
	SSX_DBG_TRACE_TOPO = 17   /* in: orig[3], dir[3], ignore quad (int), has_ray (0 / 1)   out: as SSX_DBG_TRACE */
};
/* rng[4] = PCG32 {state lo, state hi, inc lo, inc hi} */
/* ssx_debug_sweep: device-side comparison of a cheaper device function with the function that DEFINES the
 * result, over the 32-bit patterns [lo, lo+count) (count up to 2^32 = every float): result[0] = number of
 * inputs with a different result (NaN matches NaN), result[1] = op-specific maximum, result[2] = examples
 * stored, result[3..10] = mismatching inputs. */
enum {
	SSX_SWEEP_RCP = 1,         /* ssx_exact::rcp(x) vs 1.0f / x */
	SSX_SWEEP_SQRT = 2,        /* ssx_exact::sqrt_normal(x) vs sqrtf(x) */
	SSX_SWEEP_INVERSESQRT = 3, /* the kernel's inversesqrt vs 1.0f / sqrtf(x) (glm::inversesqrt) */
	SSX_SWEEP_SIN = 4,         /* kernel variant of ssx_sinf vs include/ssx_fmath.h */
	SSX_SWEEP_COS = 5,
	SSX_SWEEP_ACOS = 6,
	SSX_SWEEP_DIV_PI = 7,      /* x / pi_f through the binary64 reciprocal constant vs IEEE division */
	SSX_SWEEP_RCP64 = 8,       /* binary64 reciprocal of a float: result[1] = largest error in ulps of 1.0 / (double)x */
	SSX_SWEEP_DIV_PAIRS = 9,   /* x / hash(x), x / (hash with x's exponent), hash(x) / x through div64 vs IEEE division */
	SSX_SWEEP_ACOS_SIN = 10,   /* |x| <= 1: fused {min(acos x, under_pi), its sine} vs ssx_acosf / ssx_sinf; result[1] = inputs sent to the fallback */
	/* include/ssx_fmath.h against an INDEPENDENT evaluation (csrc/ssx_ddmath.h: double-double Taylor series, three-part pi/2, Newton on
	 * the cosine -- nothing shared with the header), every float pattern: result[0] = inputs where ssx_*f is not the correctly rounded
	 * value the independent evaluation decides on (or not NaN outside the domain; for sin and cos also: where ssx_sincosf returns another
	 * float than ssx_sinf / ssx_cosf), result[1] = inputs whose value lies within 2^-70 of a
	 * float rounding boundary, which it does not decide; examples (result[3..]): the input pattern, | 1 << 32 for an undecided one */
	SSX_SWEEP_SIN_PROOF = 11, SSX_SWEEP_COS_PROOF = 12, SSX_SWEEP_ACOS_PROOF = 13,
	/* libm = glibc-2.35, run with the LDS table of the _glibc kernels.  Digests of include/ssx_glibc_math.h as the device evaluates it, for the
	 * host to recompute with the same header: result[1] = sum over the patterns x of splitmix64(x << 32 | f(x)) mod 2^64, any NaN result
	 * counted as 0x7FC00000; result[0] = inputs where ssx_glibc_sincosf returns another float than ssx_glibc_sinf / ssx_glibc_cosf. */
	SSX_SWEEP_GLIBC_SIN = 14, SSX_SWEEP_GLIBC_COS = 15, SSX_SWEEP_GLIBC_ACOS = 16,
	SSX_SWEEP_GLIBC_COS_LDS = 17 /* the one ssx_fmath.h function the _glibc kernels keep (ssx_cosf_lds, random.cpp:134) with their LDS
	                                table vs ssx_cosf: result[0] = mismatches */
};
int ssx_debug_sweep(ssx_ctx* ctx, uint32_t op, uint32_t lo, uint64_t count, uint64_t result[11]);
/* The text of the pass-1 function ssx_set_jit would compile for the sharing pattern vid[n_quads][4] (distinct-vertex ids of
 * v00, v10, v11, v01, numbered by first occurrence), under the name pass1_<name>: returns its length (and copies up to
 * out_size - 1 characters).  Needs no device: the CPU tests compare it with what tools/gen_pass1.py wrote into
 * csrc/ssx_pass1_gen.h for the built-in topologies. */
int ssx_debug_pass1_source(const uint8_t* vid, uint32_t n_quads, const char* name, char* out, size_t out_size);
int ssx_debug_eval(ssx_ctx* ctx, uint32_t op, const void* in, uint32_t in_words, void* out, uint32_t out_words, uint32_t n);
/* One launch of the whole image (tile_first 0, tile_stride 1), per-sample results in [j][i][k] order:
 * xyza = what Renderer::_render_sample returns (float4), rng_state = the sample's PCG32 state after its
 * last draw (i.e. the number of draws consumed), levels = continued recursion levels.  Any may be NULL. */
int ssx_debug_samples(ssx_ctx* ctx, const ssx_render_params* params, float* xyza, uint64_t* rng_state, uint32_t* levels);
/* The same launch with spectral output on (ssx_set_spectral_bins; off: SSX_ERR_STATE): flux [j][i][k][4] = every sample's hero flux as handed to
 * flux_to_xyz, lambda_0 [j][i][k] = its first hero wavelength.  Either may be NULL. */
int ssx_debug_sample_flux(ssx_ctx* ctx, const ssx_render_params* params, float* flux, float* lambda_0);
/* The per-tile primitive masks the generate kernel's trace is restricted to where camera rays are pre-traced (ssx_calibration_info): exactly
 * ssx_tile_mask_kernel, launched for the plan a render with `params` gets (tile_first / tile_stride / tile_skew included; spp is not looked at),
 * whichever way the uploaded scene traces its camera rays.  out: 4 words per tile slot of the device (slot s = tile tile_first + s * tile_stride of
 * the skewed tile list), word g = primitives 32 g .. 32 g + 31.  Touches neither the sample arrays nor the sums: the continuable state stays. */
int ssx_debug_tile_mask(ssx_ctx* ctx, const ssx_render_params* params, uint32_t* out);
/* SAMPLE GENERATION, the first stage of a render, read back: ssx_generate_kernel -- the kernel a render launches, through the launch path a render takes
 * (the plan a render with `params` gets, ssx_tile_mask_kernel first where camera rays are pre-traced) -- for samples [k0, k0 + n_k) of every pixel of the
 * device's tiles (tile_first / tile_stride / tile_skew of `params`; its spp is only checked).  No path kernel runs.  pre_hits: 1 = trace the camera rays
 * (SSX_PRE_HITS=1's mode), 0 = leave them to the path loop, -1 = what the uploaded scene's calibration chose (ssx_calibration_info).
 * Records come back in the kernel's own order, [tile slot][k - k0][pixel of the tile: 8 * row + column], 4 words each:
 *   ray = {camera ray direction [3] (binary64 arithmetic, rounded once), lambda_0 (0 in RGB mode)}
 *   st  = the sample's PCG32 {state lo, state hi, inc lo, inc hi} after its draws (two for the sub-pixel, one for lambda_0 unless RGB mode) -- or, with
 *         pre_hits and a ray that leaves the scene, the end-of-path form the fold reads: {bits of lambda_0, tail word (no hit, no emission, zero levels,
 *         previous slot 0x1FFF), state lo, state hi}
 *   hit = pre_hits only: {dist, st.x, st.y, 2 * primitive + triangle as int bits}; st is +0 unless the primitive's albedo is a texture; a ray that leaves
 *         the scene has {+inf, 0, 0, -1}
 * The three arrays are the call's own and are filled with the byte SSX_GENERATE_FILL_BYTE before the launch, so a word that no lane wrote comes back as
 * 0xA6A6A6A6: all of hit[] without pre_hits, and every record of a lane outside a ragged image.  No record a lane writes is the fill in all its words: as a
 * float the word is negative, and ray's lambda_0, hit's dist and the end-of-path st's first word are not; a live st's third word is odd (inc), the fill even.
 * ray, st: [owned tiles * n_k * 64][4]; hit: the same, may be NULL unless camera rays are pre-traced.  Touches neither the context's sample arrays nor its
 * sums: a render can be continued across the call.
 * SSX_ERR_ARG with a message: n_k == 0; k0 + n_k beyond 32 bits; pre_hits outside -1..1; hit == NULL where camera rays are pre-traced; more samples per
 * pixel than one launch of that plan may cover (its sample arrays' budget, at most 65536). */
#define SSX_GENERATE_FILL_BYTE 0xA6u
int ssx_debug_generate(ssx_ctx* ctx, const ssx_render_params* params, uint32_t k0, uint32_t n_k, int pre_hits,
                       float* ray /* [n_rec][4] */, uint32_t* st /* [n_rec][4] */, float* hit /* [n_rec][4] or NULL */);
/* ssx_spectral_bin_kernel and, with q given, ssx_spectral_moment_kernel -- the very kernels a render launches after each launch of its sample walk, through the
 * launch helpers the render uses -- on sample records the caller supplies, as a pure function of its arguments (no scene needed, like ssx_probe_arrays).  n_k
 * [launches]: the samples per pixel of each launch, K their sum; flux [height][width][K][4]: every sample's hero flux; lambda_0 [height][width][K]: its first hero
 * wavelength (to be kept within [lambda_min, lambda_min + lambda_step]: outside it the index of "Spectral radiance output" is not defined).  From S, N, Q zeroed
 * as ssx_render_start leaves them, launch l hands the kernels samples [k0, k0 + n_k[l]) of every pixel the tile list of tile_first / tile_stride / tile_skew
 * owns, laid out as the path kernels leave them ([tile slot][k - k0][pixel of the tile]); then the export and variance kernels bring back sums [height][width][bins],
 * counts [height][width][bins / 4] and q [height][width][bins] (the raw second-moment sums of ssx_spectral_variance; may be NULL: the moment kernel does not
 * run).  Pixels of other tiles come back as +0.0 / 0.  The bits are those of "Spectral radiance output" and "Spectral moments" restated sequentially in ascending
 * k, whatever the split into launches (tests/spectral_accumulate_cases.py).  It touches nothing of the context's: sums, bins, moments and what is valid stay.
 * SSX_ERR_ARG, ssx_last_error naming the field: bins not a multiple of 4 in 4..64; an empty or too large image, or more than 2^30 records (tiles * 64 * K);
 * tile_stride == 0 or tile_first >= tile_stride; lambda_min not finite, lambda_step not finite and positive; launches == 0 or an n_k of 0; a NULL n_k, flux,
 * lambda_0, sums or counts.  SSX_ERR_STATE: a render runs. */
int ssx_debug_spectral_accumulate(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, uint32_t tile_first, uint32_t tile_stride, uint32_t tile_skew,
                                  float lambda_min, float lambda_step, uint32_t launches, const uint32_t* n_k /* [launches] */,
                                  const float* flux /* [H][W][K][4] */, const float* lambda_0 /* [H][W][K] */,
                                  double* sums /* [H][W][B] */, uint32_t* counts /* [H][W][M] */, double* q /* [H][W][B] or NULL */);
/* The path kernel's FOLD on levels the caller supplies: what a render computes from a path's logged levels once every ray is traced -- the way back up of
 * the recursion (renderer.cpp:147-255: per level emission + next-event term + ((radiance below * n_dot_l) * f_s) / pdf), the flat-field multiply, flux -> XYZ,
 * alpha, and the pixel's binary64 sums (renderer.cpp:292-295) in ascending k.  A sample is one row of SSX_FOLD_ROW_WORDS 32-bit words, independent of the log
 * layout (the oracle's orc_fold_sample is the same row):
 *   lambda_0 | camera ray direction [3] | hit anything (0 / 1) | n = continued levels, 0..9 | 4 words not read | level 0 .. level 9, each
 *   f_s[4], n_dot_l, pdf | flags | emission[4] | next-event term[4]
 * Level n is the path's last; only the levels below it use f_s, n_dot_l, pdf; levels above n are not read.  flags: SSX_FOLD_EMISSION, SSX_FOLD_NEE (the level
 * parked a shadow ray for this term), SSX_FOLD_NEE_VISIBLE (the ray reached its light).
 * levels: [n_pixels][spp] rows, n_pixels a multiple of 64, spp in 1..8.  One wave takes 64 pixels: it writes the rows into a log region of the call's own with the
 * functions the path kernel's write side calls, the wide or narrow queue entries' way, and folds one cohort per pass as a work unit's wave does -- the kernel twin
 * (queue entries, libm, flux) a render of this context with `params` would run, and `params`' switches (no_flat_field_correction; width, height and spp are only
 * checked).  order_seed: the order in which a cohort's log slots are handed out (any value gives the same results).  parked = 0: the samples are added as they are
 * folded; 1: they are parked as a unit's are whose turn has not come, and added from there in ascending k.
 * out_flux [n_pixels][spp][4]: the hero flux handed to flux -> XYZ (NULL, or with spectral output on: ssx_set_spectral_bins; otherwise SSX_ERR_STATE);
 * out_xyza [n_pixels][spp][4]; out_sums [n_pixels][4] binary64, from +0.0.  Either may be NULL.  Touches none of the context's render state.
 * SSX_ERR_ARG: n_pixels no multiple of 64 or above 2^20, spp outside 1..8, parked above 1, or so many pixels and samples that the call's level logs would reach
 * 4 GiB (the kernels address them with 32-bit offsets; 582 bytes per pixel, cohort and sample of the cohort, twice). */
#define SSX_FOLD_ROW_WORDS 160u
#define SSX_FOLD_LAMBDA0 0u
#define SSX_FOLD_CAM_DIR 1u
#define SSX_FOLD_HIT 4u
#define SSX_FOLD_N 5u
#define SSX_FOLD_LEVEL0 10u
#define SSX_FOLD_LEVEL_WORDS 15u
#define SSX_FOLD_L_FS 0u
#define SSX_FOLD_L_NDL 4u
#define SSX_FOLD_L_PDF 5u
#define SSX_FOLD_L_FLAGS 6u
#define SSX_FOLD_L_EMISSION 7u
#define SSX_FOLD_L_NEE 11u
#define SSX_FOLD_EMISSION 1u
#define SSX_FOLD_NEE 2u
#define SSX_FOLD_NEE_VISIBLE 4u
int ssx_debug_fold(ssx_ctx* ctx, const ssx_render_params* params, uint32_t n_pixels, uint32_t spp, const uint32_t* levels, uint32_t order_seed, uint32_t parked,
                   float* out_flux, float* out_xyza, double* out_sums);
/* The path kernel's STEP on rays the caller supplies: one level of L() (renderer.cpp:147-255) per row, as one iteration of the path kernel's loop runs it --
 * trace<TOPO> of the ray, hit_st where the hit quad's albedo is a texture, path_step (emission, light sample, parked shadow ray, BSDF sample, the level's
 * entry), the end of a path that ends (its tail word), and the flush of the parked shadow rays (shadow_flush, through the loop a render's flush runs) -- in
 * kernels of their own, the twin (topology 0 / 1 / 2, queue entries, libm) a render of this context with `params` would run; `params`' switches
 * no_explicit_light_sampling and indirect_only are honoured (width, height, spp are only checked), the SSX_NARROW_QUEUE switch too.
 * Topology 3 (kernels compiled for the scene's own pattern) is refused with SSX_ERR_STATE: its path_step is the BLACK = true instance that topologies 0 and 2
 * run here, and its trace is SSX_DBG_TRACE_TOPO's.
 * rows: [n_tiles][n_rounds][64][SSX_STEP_ROW_WORDS] -- a row is one lane's path in front of the trace: ray origin[3], direction[3], quad to ignore (-1: none),
 * depth, lambda_0, PCG32 {state, inc} as four words, prev_slot (the slot of the level below's entry, SSX_STEP_NO_SLOT at depth 0; carried, never followed).
 * One wave takes a tile; round k of a tile is sample k of its 64 pixels (the level logs' cohorts, regions and record indices are a render's).  After every
 * round the wave flushes as a render does (64 or more parked rays: a wave's worth from the top of the queue), after the last round it drains the queue.
 * out: [n_tiles][n_rounds][64][SSX_STEP_OUT_WORDS], read back THROUGH THE LEVEL LOGS AND THE TAIL WORD, as the fold reads them, after the last flush:
 *   flags (SSX_STEP_HIT | _CONTINUED | _EMISSION | _PARKED | _VISIBLE) | hit triangle (2 * quad + which; -1), distance, the st handed to path_step [2] |
 *   emission[4] | the next-event term as logged [4] (narrow entries: the parked term; wide: the finished term) | the term the fold adds [4] (nee_term) |
 *   f_s[4], n_dot_l, pdf, prev_slot of the level's entry (continued rows) | the tail word's depth, hit-anything and prev_slot (ended rows) |
 *   next ray origin[3], direction[3], quad to ignore, depth | PCG32 state [2] | slot of the level's entry (which slot a row gets is immaterial)
 * SSX_ERR_ARG (ssx_last_error names the field): n_rows 0, no multiple of 64 or of 64 * n_rounds, or more than 65536 tiles; n_rounds outside 1..8 (the samples per
 * pixel of a work unit: SSX_COHORT_KS x unit_cohorts); a row's depth >= 10, ignore neither -1 nor a quad of the
 * scene, prev_slot above SSX_STEP_NO_SLOT, lambda_0 outside [lambda_min, lambda_min + lambda_step] of the scene, or level logs of 4 GiB or more. */
#define SSX_STEP_ROW_WORDS 16u
#define SSX_STEP_R_ORIG 0u
#define SSX_STEP_R_DIR 3u
#define SSX_STEP_R_IGNORE 6u
#define SSX_STEP_R_DEPTH 7u
#define SSX_STEP_R_LAMBDA0 8u
#define SSX_STEP_R_RNG 9u
#define SSX_STEP_R_PREV_SLOT 13u
#define SSX_STEP_NO_SLOT 0x1FFFu
#define SSX_STEP_OUT_WORDS 40u
#define SSX_STEP_O_FLAGS 0u
#define SSX_STEP_O_HIT_TRI 1u
#define SSX_STEP_O_HIT_DIST 2u
#define SSX_STEP_O_HIT_ST 3u
#define SSX_STEP_O_EMISSION 5u
#define SSX_STEP_O_NEE 9u
#define SSX_STEP_O_NEE_TERM 13u
#define SSX_STEP_O_FS 17u
#define SSX_STEP_O_NDL 21u
#define SSX_STEP_O_PDF 22u
#define SSX_STEP_O_PREV_SLOT 23u
#define SSX_STEP_O_TAIL_DEPTH 24u
#define SSX_STEP_O_TAIL_HIT 25u
#define SSX_STEP_O_NEXT_ORIG 26u
#define SSX_STEP_O_NEXT_DIR 29u
#define SSX_STEP_O_NEXT_IGNORE 32u
#define SSX_STEP_O_NEXT_DEPTH 33u
#define SSX_STEP_O_RNG 34u
#define SSX_STEP_O_SLOT 36u
#define SSX_STEP_HIT 1u
#define SSX_STEP_CONTINUED 2u
#define SSX_STEP_EMISSION 4u
#define SSX_STEP_PARKED 8u
#define SSX_STEP_VISIBLE 16u
int ssx_debug_step(ssx_ctx* ctx, const ssx_render_params* params, uint32_t n_rows /* n_tiles * n_rounds * 64 */, uint32_t n_rounds, const uint32_t* rows, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* SSX_H */
