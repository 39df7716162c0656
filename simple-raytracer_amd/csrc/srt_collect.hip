// srt_collect.hip — what happens to a frame AFTER the trace kernel, beyond one blocking device:
//
//  * collecting the row partition of a multi-GPU frame on one GPU: ONE ncclGather (RCCL over xGMI) of the
//    packed per-rank canvases, then an unpermute kernel on the root -- for one process per GPU
//    (srt_comm_*, srt_gather) and for one process driving several GPUs (srt_group_*, what a C++ front-end
//    that keeps the reference's `Tracer` class needs). New work: the reference is single-device
//    (/root/reference/src/tracer.cpp:13).
//  * a two-deep frame pipeline for the interactive loop (/root/reference/src/main.cpp:277-337): frame N's
//    read-back overlaps frame N+1's trace (srt_render_pipelined).
//
// RCCL is loaded with dlopen at first use, so libsrt_hip.so has no link-time dependency on it and a
// single-GPU user never touches it.
#include <dlfcn.h>

#include <cmath>
#include <cstring>
#include <new>

#include "srt_internal.h"

// ---------------------------------------------------------------------------------
// RCCL entry points (signatures of /opt/rocm/include/rccl/rccl.h)
// ---------------------------------------------------------------------------------
namespace {
typedef struct ncclComm *ncclComm_t;
struct ncclUniqueId {
	char internal[SRT_COMM_ID_BYTES];
};
static_assert(SRT_COMM_ID_BYTES == 128, "NCCL_UNIQUE_ID_BYTES");
constexpr int kNcclSuccess = 0, kNcclFloat = 7;

struct Rccl {
	void *lib = nullptr;
	int (*GetUniqueId)(ncclUniqueId *) = nullptr;
	int (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
	int (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
	int (*CommDestroy)(ncclComm_t) = nullptr;
	int (*Gather)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
	int (*GroupStart)() = nullptr;
	int (*GroupEnd)() = nullptr;
	const char *(*GetErrorString)(int) = nullptr;
	std::string error;
};

Rccl &rccl() {
	static Rccl r;
	return r;
}

bool rccl_load() {
	Rccl &r = rccl();
	if (r.lib) return true;
	for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
		r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
		if (r.lib) break;
	}
	if (!r.lib) {
		r.error = std::string("RCCL not found (dlopen librccl.so.1): ") + (dlerror() ? dlerror() : "");
		return false;
	}
	auto sym = [&](const char *n) { return dlsym(r.lib, n); };
	r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
	r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
	r.CommInitAll = reinterpret_cast<decltype(r.CommInitAll)>(sym("ncclCommInitAll"));
	r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
	r.Gather = reinterpret_cast<decltype(r.Gather)>(sym("ncclGather"));
	r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(sym("ncclGroupStart"));
	r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(sym("ncclGroupEnd"));
	r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
	if (!r.GetUniqueId || !r.CommInitRank || !r.CommInitAll || !r.CommDestroy || !r.Gather || !r.GroupStart || !r.GroupEnd || !r.GetErrorString) {
		r.error = "librccl.so lacks an entry point this library needs (ncclGather and friends)";
		dlclose(r.lib);
		r.lib = nullptr;
		return false;
	}
	return true;
}

#define SRT_NCCL(t, call)                                                                                        \
	do {                                                                                                         \
		int r_ = (call);                                                                                         \
		if (r_ != kNcclSuccess) return fail((t), SRT_ERR_HIP, std::string(#call) + ": " + rccl().GetErrorString(r_)); \
	} while (0)
} // namespace

// per-handle state of this module
struct SrtCollect {
	ncclComm_t comm = nullptr;
	bool comm_owned = false; // created by srt_comm_init (else by a group's ncclCommInitAll)
	int comm_rank = -1, comm_world = 0;
	DevBuf<float> gathered; // root: world x padded_rows x width float4, rank-major
	DevBuf<float> full;     // root: height x width float4, the unpermuted image
	DevBuf<uint8_t> full_argb;
	bool have_full = false;
	// frame pipeline
	hipStream_t copy_stream = nullptr;
	uint8_t *pinned[2] = {nullptr, nullptr};
	uint8_t *dev_argb[2] = {nullptr, nullptr};
	size_t frame_bytes = 0;
	hipEvent_t resolved[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
	long long frames_enqueued = 0, frames_delivered = 0;
};

namespace {
SrtCollect *collect_of(srt_tracer *t) {
	if (!t->collect) t->collect = new (std::nothrow) SrtCollect();
	return t->collect;
}

// image row y of the frame <- packed row of the rank that owns it (include/srt_abi.h srt_set_partition)
__global__ __launch_bounds__(256) void srt_unpermute_kernel(const float4 *__restrict__ gathered, float4 *__restrict__ image, int width, int height,
                                                            int world, int rpb, int padded_rows) {
	const size_t n = (size_t)width * height;
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
		const int y = (int)(i / width), x = (int)(i - (size_t)y * width);
		const int blk = y / rpb, r = blk % world, lb = blk / world;
		const int lr = lb * rpb + (y - blk * rpb);
		image[i] = gathered[((size_t)r * padded_rows + lr) * width + x];
	}
}

// The same for a frame gathered with the denoiser's inputs (srt_group_set_denoise): every rank's slot of `gathered` is
// gd_slot_floats(plane) floats -- three float4 planes of `plane` = padded_rows * width pixels (canvas rows, normal_depth,
// albedo_hits) and one float plane (moments) -- and ONE pass puts all four back in image order, a pixel's 52 bytes per lane.
__global__ __launch_bounds__(256) void srt_unpermute_planes_kernel(const float *__restrict__ gathered, float4 *__restrict__ canvas,
                                                                   float4 *__restrict__ normal_depth, float4 *__restrict__ albedo_hits,
                                                                   float *__restrict__ moments, int width, int height, int world, int rpb,
                                                                   int padded_rows, size_t slot_floats) {
	const size_t n = (size_t)width * height, plane = (size_t)padded_rows * width;
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
		const int y = (int)(i / width), x = (int)(i - (size_t)y * width);
		const int blk = y / rpb, r = blk % world, lb = blk / world;
		const int lr = lb * rpb + (y - blk * rpb);
		const float *__restrict__ slot = gathered + (size_t)r * slot_floats;
		const float4 *__restrict__ slot4 = reinterpret_cast<const float4 *>(slot);
		const size_t j = (size_t)lr * width + x; // < plane: lr < padded_rows
		canvas[i] = slot4[j];
		normal_depth[i] = slot4[plane + j];
		albedo_hits[i] = slot4[2 * plane + j];
		moments[i] = slot[12 * plane + j];
	}
}

int launch_unpermute_planes(const float *gathered, float *canvas, float *nd, float *ah, float *mom, int width, int height, int world, int rpb,
                            hipStream_t stream) {
	const int padded = srt_partition_padded_rows(height, world, rpb);
	const size_t n = (size_t)width * height;
	unsigned blocks = (unsigned)((n + 255) / 256);
	if (blocks > 8192) blocks = 8192;
	hipLaunchKernelGGL(srt_unpermute_planes_kernel, dim3(blocks), dim3(256), 0, stream, gathered, reinterpret_cast<float4 *>(canvas),
	                   reinterpret_cast<float4 *>(nd), reinterpret_cast<float4 *>(ah), mom, width, height, world, rpb, padded,
	                   gd_slot_floats((size_t)padded * width));
	return hipGetLastError() == hipSuccess ? SRT_OK : SRT_ERR_HIP;
}

int unpermute_on_root(srt_tracer *t, SrtCollect *c) {
	const int padded = srt_partition_padded_rows(t->height, t->world, t->rows_per_block);
	const size_t n = (size_t)t->width * t->height;
	SRT_HIP(t, c->full.reserve(n * 4));
	unsigned blocks = (unsigned)((n + 255) / 256);
	if (blocks > 8192) blocks = 8192;
	hipLaunchKernelGGL(srt_unpermute_kernel, dim3(blocks), dim3(256), 0, t->stream, reinterpret_cast<const float4 *>(c->gathered.ptr),
	                   reinterpret_cast<float4 *>(c->full.ptr), t->width, t->height, t->world, t->rows_per_block, padded);
	SRT_HIP(t, hipGetLastError());
	c->have_full = true;
	return SRT_OK;
}
} // namespace

void srt_collect_release(srt_tracer *t) {
	SrtCollect *c = t->collect;
	if (!c) return;
	if (c->comm && c->comm_owned && rccl().lib) (void)rccl().CommDestroy(c->comm);
	c->gathered.release();
	c->full.release();
	c->full_argb.release();
	if (c->copy_stream) {
		(void)hipStreamSynchronize(c->copy_stream);
		(void)hipStreamDestroy(c->copy_stream);
	}
	for (int i = 0; i < 2; i++) {
		if (c->pinned[i]) (void)hipHostFree(c->pinned[i]);
		if (c->dev_argb[i]) (void)hipFree(c->dev_argb[i]);
		if (c->resolved[i]) (void)hipEventDestroy(c->resolved[i]);
		if (c->copied[i]) (void)hipEventDestroy(c->copied[i]);
	}
	delete c;
	t->collect = nullptr;
}

extern "C" {

// ---------------------------------------------------------------------------------
// one process per GPU
// ---------------------------------------------------------------------------------
int srt_comm_unique_id(void *id_out) {
	if (!id_out) return SRT_ERR_INVALID;
	if (!rccl_load()) return fail(nullptr, SRT_ERR_HIP, rccl().error);
	ncclUniqueId id;
	SRT_NCCL(nullptr, rccl().GetUniqueId(&id));
	memcpy(id_out, id.internal, SRT_COMM_ID_BYTES);
	return SRT_OK;
}

int srt_comm_init(srt_tracer *t, const void *id, int rank, int world) {
	if (!t) return SRT_ERR_INVALID;
	if (!id || world < 1 || rank < 0 || rank >= world) return fail(t, SRT_ERR_INVALID, "srt_comm_init: need an id and 0 <= rank < world");
	if (!rccl_load()) return fail(t, SRT_ERR_HIP, rccl().error);
	SrtCollect *c = collect_of(t);
	if (!c) return fail(t, SRT_ERR_INVALID, "out of host memory");
	if (c->comm) return fail(t, SRT_ERR_STATE, "srt_comm_init: the handle already has a communicator");
	SRT_HIP(t, hipSetDevice(t->device));
	ncclUniqueId uid;
	memcpy(uid.internal, id, SRT_COMM_ID_BYTES);
	SRT_NCCL(t, rccl().CommInitRank(&c->comm, world, uid, rank));
	c->comm_owned = true;
	c->comm_rank = rank;
	c->comm_world = world;
	return SRT_OK;
}

int srt_gather(srt_tracer *t, int root) {
	if (!t) return SRT_ERR_INVALID;
	SrtCollect *c = t->collect;
	if (!c || !c->comm) return fail(t, SRT_ERR_STATE, "srt_gather: no communicator (srt_comm_init)");
	if (c->comm_world != t->world || c->comm_rank != t->rank)
		return fail(t, SRT_ERR_STATE, "srt_gather: the communicator's rank / world differ from srt_set_partition's");
	if (root < 0 || root >= t->world) return fail(t, SRT_ERR_INVALID, "srt_gather: root out of range");
	SRT_HIP(t, hipSetDevice(t->device));
	const int padded = srt_partition_padded_rows(t->height, t->world, t->rows_per_block);
	const size_t count = (size_t)padded * t->width * 4; // floats every rank sends (its canvas buffer holds padded rows)
	if (t->canvas_bytes < count * sizeof(float)) return fail(t, SRT_ERR_STATE, "srt_gather: canvas smaller than padded_rows * width * 16 (bind a larger one)");
	if (t->rank == root) SRT_HIP(t, c->gathered.reserve(count * (size_t)t->world));
	// the ONE collective of the path: every peer's packed canvas over its own xGMI link to the root
	SRT_NCCL(t, rccl().Gather(t->canvas, t->rank == root ? c->gathered.ptr : nullptr, count, kNcclFloat, root, c->comm, t->stream));
	if (t->rank == root) return unpermute_on_root(t, c);
	return SRT_OK;
}

/* test hook: the unpermute kernel alone on caller-owned device buffers (gathered: world x padded_rows x width float4,
 * image: height x width float4), on the NULL stream, synchronous */
int srt_unpermute_device(const void *gathered, void *image, int width, int height, int world, int rows_per_block) {
	if (!gathered || !image || width <= 0 || height <= 0 || world < 1 || rows_per_block < 1) return SRT_ERR_INVALID;
	const int padded = srt_partition_padded_rows(height, world, rows_per_block);
	const size_t n = (size_t)width * height;
	unsigned blocks = (unsigned)((n + 255) / 256);
	if (blocks > 8192) blocks = 8192;
	hipLaunchKernelGGL(srt_unpermute_kernel, dim3(blocks), dim3(256), 0, nullptr, static_cast<const float4 *>(gathered), static_cast<float4 *>(image),
	                   width, height, world, rows_per_block, padded);
	if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return SRT_ERR_HIP;
	return SRT_OK;
}

/* test hook: the multi-plane unpermute kernel alone on caller-owned device buffers (gathered: world slots of
 * srt_partition_planes_floats() floats; canvas, normal_depth, albedo_hits: height x width float4; moments: height x width
 * float), on the NULL stream, synchronous */
int srt_unpermute_planes_device(const void *gathered, void *canvas, void *normal_depth, void *albedo_hits, void *moments, int width, int height,
                                int world, int rows_per_block) {
	if (!gathered || !canvas || !normal_depth || !albedo_hits || !moments || width <= 0 || height <= 0 || world < 1 || rows_per_block < 1)
		return SRT_ERR_INVALID;
	if (launch_unpermute_planes(static_cast<const float *>(gathered), static_cast<float *>(canvas), static_cast<float *>(normal_depth),
	                            static_cast<float *>(albedo_hits), static_cast<float *>(moments), width, height, world, rows_per_block, nullptr) != SRT_OK ||
	    hipDeviceSynchronize() != hipSuccess)
		return SRT_ERR_HIP;
	return SRT_OK;
}

long long srt_partition_planes_floats(int width, int height, int world, int rows_per_block) {
	if (width <= 0 || height < 0 || world < 1 || rows_per_block < 1) return -1;
	return (long long)gd_slot_floats(gd_plane_pixels(width, height, world, rows_per_block));
}

int srt_resolve_gathered(srt_tracer *t, uint32_t ticks_stopped) {
	if (!t) return SRT_ERR_INVALID;
	SrtCollect *c = t->collect;
	if (!c || !c->have_full) return fail(t, SRT_ERR_STATE, "srt_resolve_gathered: nothing gathered on this handle (srt_gather as root)");
	const size_t n = (size_t)t->width * t->height;
	SRT_HIP(t, c->full_argb.reserve(n * 4));
	if (const int rc = srt_resolve_external(t, c->full.ptr, (uint32_t)n, ticks_stopped, c->full_argb.ptr)) return rc;
	// exposure.hip, bloom.hip: nothing while the features are off; the gathered frame is a picture
	if (const int rc = srt_exposure_apply(t, c->full.ptr, (float)ticks_stopped, (uint32_t)t->width, (uint32_t)t->height, true, c->full_argb.ptr)) return rc;
	return srt_selection_apply(t, (uint32_t)t->width, (uint32_t)t->height, true, c->full_argb.ptr); // selection.hip: likewise, the last step on the bytes
}

int srt_gathered_buffers(srt_tracer *t, void **canvas, void **argb) {
	if (!t) return SRT_ERR_INVALID;
	SrtCollect *c = t->collect;
	if (!c || !c->have_full) return fail(t, SRT_ERR_STATE, "srt_gathered_buffers: nothing gathered on this handle");
	if (canvas) *canvas = c->full.ptr;
	if (argb) *argb = c->full_argb.ptr;
	return SRT_OK;
}

int srt_read_gathered(srt_tracer *t, float *canvas_out, uint8_t *argb_out) {
	if (!t) return SRT_ERR_INVALID;
	SrtCollect *c = t->collect;
	if (!c || !c->have_full) return fail(t, SRT_ERR_STATE, "srt_read_gathered: nothing gathered on this handle");
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t n = (size_t)t->width * t->height;
	if (canvas_out) SRT_HIP(t, hipMemcpyAsync(canvas_out, c->full.ptr, n * 16, hipMemcpyDeviceToHost, t->stream));
	if (argb_out) {
		if (c->full_argb.cap < n * 4) return fail(t, SRT_ERR_STATE, "srt_read_gathered: no resolved image (srt_resolve_gathered)");
		SRT_HIP(t, hipMemcpyAsync(argb_out, c->full_argb.ptr, n * 4, hipMemcpyDeviceToHost, t->stream));
	}
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

} // extern "C"

// ---------------------------------------------------------------------------------
// one process, several GPUs: what `Tracer(width, height, n_devices)` of host/tracer.hpp drives
// ---------------------------------------------------------------------------------
struct srt_group {
	std::vector<srt_tracer *> t;
	int width = 0, height = 0, rpb = 8;
	// The device list names a device more than once ("virtual devices": N members on fewer GPUs, down to one). RCCL refuses such a
	// list, and there is no link to cross: the collection is then a device-to-device copy of every member's packed canvas into its
	// slot of the root's buffer, enqueued on the member's own stream where ncclGather would be, and the root's stream waits for all
	// of them before it unpermutes. Partition, packed layout, unpermute, resolve and every srt_group_* call are the real ones --
	// what a one-GPU box can run of the N > 1 path (tests/test_gpu_collect.py).
	bool loopback = false;
	std::vector<hipEvent_t> copied; // loopback: member i's canvas has arrived in the root's buffer
	// The denoiser on a group (srt_group_set_denoise). The members accumulate the filter's inputs for their own rows
	// (srt_internal.h "group denoiser"), one collective brings canvas rows and inputs to the root, one unpermute puts them into
	// the full-frame state of `resolver`: a handle of the whole frame on the root device and the root's stream, made when the
	// denoiser is first asked for. Its canvas is the root's SrtCollect::full, its dn_nd / dn_ah / dn_mom the other planes, its
	// counts and camera the group's, its history buffers the group's only ones -- and filter, temporal set-up and commit,
	// validation and the read-backs are the single handle's code run on it.
	srt_tracer *resolver = nullptr;
	bool dn_on = false;
	int dn_feature_samples = 0;
	hipEvent_t unpermuted = nullptr;  // loopback: the root has read the gather buffer (the next frame's copies wait for it)
	std::vector<uint8_t> scene_bytes; // the last srt_group_update_scene's (the history survives an unchanged scene)
	std::string err;
};

namespace {
int gfail(srt_group *g, int code, const std::string &msg) {
	if (g) g->err = msg;
	return code;
}

// the group's full-frame handle for the denoiser, made at first use; it works on the root's stream as that is bound now
srt_tracer *resolver_of(srt_group *g) {
	srt_tracer *root = g->t[0];
	if (!g->resolver) {
		srt_tracer *r = nullptr;
		if (srt_create(g->width, g->height, root->device, &r) != SRT_OK) {
			g->err = std::string("srt_group: the denoiser's handle on the root device: ") + srt_last_error(nullptr);
			return nullptr;
		}
		// its canvas is the gathered, unpermuted one (bound the way srt_bind_canvas does); its own is not needed
		SrtCollect *rc = root->collect;
		const size_t n = (size_t)g->width * g->height;
		if (hipSetDevice(root->device) != hipSuccess || rc->full.reserve(n * 4) != hipSuccess ||
		    hipMemsetAsync(rc->full.ptr, 0, n * 16, root->stream) != hipSuccess ||
		    (g->loopback && hipEventCreateWithFlags(&g->unpermuted, hipEventDisableTiming) != hipSuccess)) {
			(void)hipGetLastError();
			srt_destroy(r);
			g->err = "srt_group: the denoiser's buffers on the root device";
			return nullptr;
		}
		r->canvas_own.release();
		r->canvas = rc->full.ptr;
		r->canvas_bytes = n * 16;
		g->resolver = r;
	}
	g->resolver->stream = root->stream;
	g->resolver->ex = root->ex; // one exposure state per group, the first member's (srt_group_set_exposure)
	g->resolver->bl = root->bl; // ... and one bloom state (srt_group_set_bloom)
	g->resolver->nz = root->nz; // ... and one noise meter (srt_group_set_noise_meter)
	g->resolver->sel = root->sel; // ... and one selection, which names the root's scene (srt_group_set_selection)
	return g->resolver;
}

// a history-dropping call reached the members: the group's history saw the old sky / textures / scene
void drop_history(srt_group *g) {
	if (g->resolver) srt_temporal_drop(g->resolver);
}
} // namespace

extern "C" {

void srt_group_destroy(srt_group *g) {
	if (!g) return;
	for (hipEvent_t e : g->copied)
		if (e) (void)hipEventDestroy(e);
	if (g->resolver) { // (its canvas is the root's gathered image: gone with the root below)
		(void)hipSetDevice(g->resolver->device);
		if (!g->t.empty() && g->t[0]) (void)hipStreamSynchronize(g->t[0]->stream);
		g->resolver->canvas = nullptr;
		srt_destroy(g->resolver);
	}
	if (g->unpermuted) (void)hipEventDestroy(g->unpermuted);
	for (srt_tracer *t : g->t) {
		if (t && t->collect && t->collect->comm && rccl().lib) {
			(void)hipSetDevice(t->device);
			(void)hipStreamSynchronize(t->stream);
			(void)rccl().CommDestroy(t->collect->comm);
			t->collect->comm = nullptr;
		}
	}
	for (srt_tracer *t : g->t) srt_destroy(t);
	delete g;
}

const char *srt_group_last_error(const srt_group *g) { return g ? g->err.c_str() : "srt_group: NULL"; }

int srt_group_create(int width, int height, int n_devices, const int *devices, int rows_per_block, srt_group **out) {
	if (!out) return SRT_ERR_INVALID;
	*out = nullptr;
	if (n_devices < 1 || rows_per_block < 1) return fail(nullptr, SRT_ERR_INVALID, "srt_group_create: need n_devices >= 1 and rows_per_block >= 1");
	srt_group *g = new (std::nothrow) srt_group();
	if (!g) return fail(nullptr, SRT_ERR_INVALID, "out of host memory");
	g->width = width, g->height = height, g->rpb = rows_per_block;
	std::vector<int> devs(n_devices);
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
		(void)hipGetLastError();
		delete g;
		return fail(nullptr, SRT_ERR_HIP, "srt_group_create: no HIP device");
	}
	// no list: devices 0 .. n-1; more members than the node has devices: they wrap around (virtual devices, see srt_group::loopback)
	for (int i = 0; i < n_devices; i++) devs[i] = devices ? devices[i] : i % ndev;
	for (int i = 0; i < n_devices && !g->loopback; i++)
		for (int k = 0; k < i; k++)
			if (devs[k] == devs[i]) g->loopback = true;
	for (int i = 0; i < n_devices; i++) {
		srt_tracer *t = nullptr;
		int rc = srt_create(width, height, devs[i], &t);
		if (rc == SRT_OK) rc = srt_set_partition(t, i, n_devices, rows_per_block);
		if (rc != SRT_OK) {
			const std::string msg = std::string("srt_group_create: device ") + std::to_string(devs[i]) + ": " + srt_last_error(rc && t ? t : nullptr);
			if (t) srt_destroy(t);
			srt_group_destroy(g);
			return fail(nullptr, rc, msg);
		}
		g->t.push_back(t);
	}
	if (g->loopback) {
		for (int i = 0; i < n_devices; i++) {
			SrtCollect *c = collect_of(g->t[i]);
			hipEvent_t ev = nullptr;
			if (!c || hipSetDevice(devs[i]) != hipSuccess || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
				(void)hipGetLastError();
				srt_group_destroy(g);
				return fail(nullptr, SRT_ERR_HIP, "srt_group_create: loopback set-up");
			}
			g->copied.push_back(ev);
			c->comm_rank = i, c->comm_world = n_devices;
		}
		*out = g;
		return SRT_OK;
	}
	if (!rccl_load()) {
		srt_group_destroy(g);
		return fail(nullptr, SRT_ERR_HIP, rccl().error);
	}
	std::vector<ncclComm_t> comms(n_devices, nullptr);
	const int r = rccl().CommInitAll(comms.data(), n_devices, devs.data());
	if (r != kNcclSuccess) {
		const std::string msg = std::string("srt_group_create: ncclCommInitAll: ") + rccl().GetErrorString(r);
		srt_group_destroy(g);
		return fail(nullptr, SRT_ERR_HIP, msg);
	}
	for (int i = 0; i < n_devices; i++) {
		SrtCollect *c = collect_of(g->t[i]);
		if (!c) {
			// the communicators not yet attached to a handle (i and above) belong to nobody: destroy them here, the attached ones
			// go with their handles in srt_group_destroy
			for (int k = i; k < n_devices; k++)
				if (comms[k]) (void)rccl().CommDestroy(comms[k]);
			srt_group_destroy(g);
			return fail(nullptr, SRT_ERR_INVALID, "out of host memory");
		}
		c->comm = comms[i];
		c->comm_owned = false; // destroyed by srt_group_destroy
		c->comm_rank = i, c->comm_world = n_devices;
	}
	*out = g;
	return SRT_OK;
}

int srt_group_size(const srt_group *g) { return g ? (int)g->t.size() : 0; }
srt_tracer *srt_group_tracer(srt_group *g, int i) { return (g && i >= 0 && i < (int)g->t.size()) ? g->t[i] : nullptr; }

#define SRT_EACH(g, expr)                                                                  \
	do {                                                                                   \
		for (srt_tracer * t_ : (g)->t) {                                                   \
			const int rc_ = (expr);                                                        \
			if (rc_ != SRT_OK) return gfail((g), rc_, srt_last_error(t_));                 \
		}                                                                                  \
	} while (0)

int srt_group_set_skybox(srt_group *g, const float *rgba, int width, int height) {
	if (!g) return SRT_ERR_INVALID;
	SRT_EACH(g, srt_set_skybox(t_, rgba, width, height));
	drop_history(g); // (as the per-handle call does for its own)
	return SRT_OK;
}

int srt_group_set_textures(srt_group *g, const srt_texture_desc *descs, size_t n) {
	if (!g) return SRT_ERR_INVALID;
	SRT_EACH(g, srt_set_textures(t_, descs, n));
	drop_history(g); // (as the per-handle call does for its own)
	return SRT_OK;
}

int srt_group_set_material_textures(srt_group *g, const srt_material_texture *bindings, size_t n_materials) {
	if (!g) return SRT_ERR_INVALID;
	SRT_EACH(g, srt_set_material_textures(t_, bindings, n_materials));
	drop_history(g); // (as the per-handle call does for its own)
	return SRT_OK;
}

int srt_group_set_triangle_uvs(srt_group *g, const float *uv, size_t n_triangles) {
	if (!g) return SRT_ERR_INVALID;
	SRT_EACH(g, srt_set_triangle_uvs(t_, uv, n_triangles));
	drop_history(g); // (as the per-handle call does for its own)
	return SRT_OK;
}

int srt_group_set_triangle_materials(srt_group *g, const int32_t *materials, size_t n_triangles) {
	if (!g) return SRT_ERR_INVALID;
	SRT_EACH(g, srt_set_triangle_materials(t_, materials, n_triangles));
	drop_history(g); // (as the per-handle call does for its own)
	return SRT_OK;
}

int srt_group_set_acceleration(srt_group *g, int mode) {
	if (!g) return SRT_ERR_INVALID;
	SRT_EACH(g, srt_set_acceleration(t_, mode));
	return SRT_OK;
}

int srt_group_set_acceleration_refit(srt_group *g, int mode) {
	if (!g) return SRT_ERR_INVALID;
	SRT_EACH(g, srt_set_acceleration_refit(t_, mode));
	return SRT_OK;
}

int srt_group_set_acceleration_deform(srt_group *g, int mode, float rebuild_ratio) {
	if (!g) return SRT_ERR_INVALID;
	SRT_EACH(g, srt_set_acceleration_deform(t_, mode, rebuild_ratio));
	return SRT_OK;
}

int srt_group_set_acceleration_build(srt_group *g, int mode, uint32_t min_triangles) {
	if (!g) return SRT_ERR_INVALID;
	SRT_EACH(g, srt_set_acceleration_build(t_, mode, min_triangles));
	return SRT_OK;
}

int srt_group_set_acceleration_build_order(srt_group *g, int order) {
	if (!g) return SRT_ERR_INVALID;
	SRT_EACH(g, srt_set_acceleration_build_order(t_, order));
	return SRT_OK;
}

int srt_group_update_scene(srt_group *g, const srt_shape *shapes, size_t n_shapes, const srt_triangle *triangles, size_t n_triangles,
                           const srt_material *materials, size_t n_materials, const srt_scene_data *scene) {
	if (!g) return SRT_ERR_INVALID;
	// the scene is replicated: prepared on the host once (hierarchy build, shape blocks, thresholds), uploaded to every member
	size_t who = 0;
	const int rc = srt_update_scene_many(g->t.data(), g->t.size(), shapes, n_shapes, triangles, n_triangles, materials, n_materials, scene, &who);
	// the denoiser's history survives only a call with the same bytes as the previous one, as on a single handle (srt_update_scene)
	try {
		std::vector<uint8_t> bytes;
		if (scene) srt_scene_bytes(bytes, shapes, n_shapes, triangles, n_triangles, materials, n_materials, scene);
		if (rc != SRT_OK || bytes.empty() || bytes != g->scene_bytes) drop_history(g);
		g->scene_bytes.swap(bytes);
	} catch (...) {
		drop_history(g);
		g->scene_bytes.clear();
		if (rc == SRT_OK) return gfail(g, SRT_ERR_INVALID, "out of host memory");
	}
	if (rc != SRT_OK) return gfail(g, rc, srt_last_error(g->t[who < g->t.size() ? who : 0]));
	return SRT_OK;
}

int srt_group_clear_canvas(srt_group *g) {
	if (!g) return SRT_ERR_INVALID;
	if (g->dn_on) {
		// what srt_clear_canvas does for a single handle: the frame being cleared becomes the history when something was traced
		// (the commit reads the gathered planes on the root), then the sums -- each member's canvas rows and planes are one
		// fill -- and the counts start again
		srt_tracer *r = resolver_of(g);
		if (!r) return SRT_ERR_HIP;
		if (hipSetDevice(r->device) != hipSuccess) return gfail(g, SRT_ERR_HIP, "srt_group_clear_canvas: hipSetDevice");
		const int rc = srt_temporal_commit(r);
		if (rc != SRT_OK) return gfail(g, rc, srt_last_error(r));
		r->dn_T = r->dn_P = r->dn_F = 0;
	}
	SRT_EACH(g, srt_clear_canvas(t_));
	return SRT_OK;
}

// trace on every device, ONE gather to device 0 of the group, unpermute there; everything asynchronous
int srt_group_trace_and_gather(srt_group *g, const srt_render_data *options) {
	if (!g) return SRT_ERR_INVALID;
	srt_tracer *res = g->dn_on ? resolver_of(g) : nullptr;
	if (g->dn_on && !res) return SRT_ERR_HIP;
	SRT_EACH(g, srt_trace(t_, options));
	srt_tracer *root = g->t[0];
	const int world = (int)g->t.size();
	const int padded = srt_partition_padded_rows(g->height, world, g->rpb);
	// floats every rank sends: its padded canvas rows; with the denoiser on its whole gd_pack, the canvas rows and the filter's
	// inputs behind them (52 B per pixel instead of 16) -- still one collective
	const size_t count = res ? gd_slot_floats((size_t)padded * g->width) : (size_t)padded * g->width * 4;
	if (res) srt_denoise_count(res, *options, g->dn_feature_samples); // the counts of the dispatch every member has just run
	SrtCollect *rc = root->collect;
	// put the gathered frame back in image order on the root: the canvas alone, or all four planes into the resolver's state
	auto unpermute = [&]() {
		if (!res) return unpermute_on_root(root, rc);
		if (launch_unpermute_planes(rc->gathered.ptr, rc->full.ptr, res->dn_nd.ptr, res->dn_ah.ptr, res->dn_mom.ptr, g->width, g->height, world, g->rpb,
		                            root->stream) != SRT_OK)
			return fail(root, SRT_ERR_HIP, "srt_group: unpermute of the gathered planes");
		rc->have_full = true;
		return (int)SRT_OK;
	};
	if (hipSetDevice(root->device) != hipSuccess || rc->gathered.reserve(count * (size_t)world) != hipSuccess)
		return gfail(g, SRT_ERR_HIP, "srt_group: gather buffer on the root device");
	if (g->loopback) {
		for (int i = 0; i < world; i++) {
			srt_tracer *t = g->t[i];
			// (denoiser: a resolve may be enqueued behind the previous frame's unpermute, so the root can still be reading the buffer)
			if (res && i > 0 && hipStreamWaitEvent(t->stream, g->unpermuted, 0) != hipSuccess) return gfail(g, SRT_ERR_HIP, "srt_group: loopback wait");
			if (hipSetDevice(t->device) != hipSuccess ||
			    hipMemcpyAsync(rc->gathered.ptr + (size_t)i * count, t->canvas, count * sizeof(float), hipMemcpyDeviceToDevice, t->stream) != hipSuccess ||
			    hipEventRecord(g->copied[i], t->stream) != hipSuccess)
				return gfail(g, SRT_ERR_HIP, "srt_group: loopback copy of a member's canvas");
		}
		(void)hipSetDevice(root->device);
		for (int i = 1; i < world; i++)
			if (hipStreamWaitEvent(root->stream, g->copied[i], 0) != hipSuccess) return gfail(g, SRT_ERR_HIP, "srt_group: loopback wait");
		const int u = unpermute();
		if (u != SRT_OK) return gfail(g, u, srt_last_error(root));
		if (res && hipEventRecord(g->unpermuted, root->stream) != hipSuccess) return gfail(g, SRT_ERR_HIP, "srt_group: loopback event");
		return SRT_OK;
	}
	int r = rccl().GroupStart();
	for (int i = 0; i < world && r == kNcclSuccess; i++) {
		srt_tracer *t = g->t[i];
		(void)hipSetDevice(t->device);
		r = rccl().Gather(t->canvas, i == 0 ? rc->gathered.ptr : nullptr, count, kNcclFloat, 0, t->collect->comm, t->stream);
	}
	const int r2 = rccl().GroupEnd();
	if (r != kNcclSuccess || r2 != kNcclSuccess) return gfail(g, SRT_ERR_HIP, std::string("srt_group: ncclGather: ") + rccl().GetErrorString(r != kNcclSuccess ? r : r2));
	(void)hipSetDevice(root->device);
	const int u = unpermute();
	if (u != SRT_OK) return gfail(g, u, srt_last_error(root));
	return SRT_OK;
}

// Tracer::render for the group: trace everywhere, gather, resolve on device 0, blocking read-back of width*height*4 bytes
int srt_group_render(srt_group *g, const srt_render_data *options, uint32_t ticks_stopped, uint8_t *argb_out) {
	if (!g) return SRT_ERR_INVALID;
	if (!argb_out) return gfail(g, SRT_ERR_INVALID, "srt_group_render: argb_out is NULL");
	int rc = srt_group_trace_and_gather(g, options);
	if (rc != SRT_OK) return rc;
	srt_tracer *root = g->t[0];
	if (g->dn_on) { // through the filter on the root (K = 0: the plain resolve's bytes)
		rc = srt_resolve_denoised(g->resolver, ticks_stopped);
		if (rc == SRT_OK) rc = srt_read_argb(g->resolver, argb_out);
		if (rc != SRT_OK) return gfail(g, rc, srt_last_error(g->resolver));
	} else {
		rc = srt_resolve_gathered(root, ticks_stopped);
		if (rc == SRT_OK) rc = srt_read_gathered(root, nullptr, argb_out);
		if (rc != SRT_OK) return gfail(g, rc, srt_last_error(root));
	}
	for (size_t i = 1; i < g->t.size(); i++) { // every device has finished its part before the call returns
		rc = srt_synchronize(g->t[i]);
		if (rc != SRT_OK) return gfail(g, rc, srt_last_error(g->t[i]));
	}
	return SRT_OK;
}

int srt_group_read_canvas(srt_group *g, float *rgba_out) {
	if (!g) return SRT_ERR_INVALID;
	const int rc = srt_read_gathered(g->t[0], rgba_out, nullptr);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

// ---- the denoiser on a group: the per-handle calls on the group's full-frame handle, the switch carried to the members ----
#define SRT_ON_RESOLVER(g, r, expr)                                  \
	do {                                                             \
		const int rc_ = (expr);                                      \
		if (rc_ != SRT_OK) return gfail((g), rc_, srt_last_error(r)); \
	} while (0)

int srt_group_set_denoise(srt_group *g, const srt_denoise_params *params) {
	if (!g) return SRT_ERR_INVALID;
	if (!params || !params->enable) {
		if (g->resolver) SRT_ON_RESOLVER(g, g->resolver, srt_set_denoise(g->resolver, nullptr)); // (drops the history, temporal off)
		if (g->dn_on) SRT_EACH(g, srt_denoise_member(t_, 0));
		g->dn_on = false;
		return SRT_OK;
	}
	srt_tracer *r = resolver_of(g);
	if (!r) return SRT_ERR_HIP;
	const bool clear = !g->dn_on || params->feature_samples != g->dn_feature_samples;
	SRT_ON_RESOLVER(g, r, srt_set_denoise(r, params)); // validation, the full-frame buffers, and on `clear` the root's sums and history
	if (clear) SRT_EACH(g, srt_denoise_member(t_, params->feature_samples)); // canvas rows and sums of every member: zero
	g->dn_on = true;
	g->dn_feature_samples = params->feature_samples;
	return SRT_OK;
}

int srt_group_set_denoise_temporal(srt_group *g, const srt_temporal_params *params) {
	if (!g) return SRT_ERR_INVALID;
	if ((!params || !params->enable) && !g->resolver) return SRT_OK;
	srt_tracer *r = resolver_of(g);
	if (!r) return SRT_ERR_HIP;
	SRT_ON_RESOLVER(g, r, srt_set_denoise_temporal(r, params));
	return SRT_OK;
}

int srt_group_set_denoise_demodulation(srt_group *g, int enable) {
	if (!g) return SRT_ERR_INVALID;
	if (!enable) {
		if (g->resolver) SRT_ON_RESOLVER(g, g->resolver, srt_set_denoise_demodulation(g->resolver, 0));
		return SRT_OK;
	}
	if (!g->dn_on) return gfail(g, SRT_ERR_STATE, "srt_group_set_denoise_demodulation: the denoiser is off (srt_group_set_denoise)");
	srt_tracer *r = resolver_of(g);
	if (!r) return SRT_ERR_HIP;
	SRT_ON_RESOLVER(g, r, srt_set_denoise_demodulation(r, 1)); // the filter runs on that handle
	return SRT_OK;
}

int srt_group_last_filter_demodulated(const srt_group *g, int *demodulated) {
	if (!g || !demodulated) return SRT_ERR_INVALID;
	*demodulated = (g->resolver && g->resolver->last_filter.demod) ? 1 : 0;
	return SRT_OK;
}

int srt_group_set_denoise_history_illumination(srt_group *g, int enable) {
	if (!g) return SRT_ERR_INVALID;
	if (!enable) {
		if (g->resolver) SRT_ON_RESOLVER(g, g->resolver, srt_set_denoise_history_illumination(g->resolver, 0));
		return SRT_OK;
	}
	if (!g->dn_on || !g->resolver)
		return gfail(g, SRT_ERR_STATE, "srt_group_set_denoise_history_illumination: temporal reprojection is off (srt_group_set_denoise_temporal)");
	SRT_ON_RESOLVER(g, g->resolver, srt_set_denoise_history_illumination(g->resolver, 1)); // the set-up runs on that handle
	return SRT_OK;
}

int srt_group_last_setup_history_illumination(srt_group *g) { return g && g->resolver && g->resolver->last_setup.illum ? 1 : 0; }

int srt_group_set_denoise_history_clamp(srt_group *g, float gamma) {
	if (!g) return SRT_ERR_INVALID;
	if (gamma == 0.0f) {
		if (g->resolver) SRT_ON_RESOLVER(g, g->resolver, srt_set_denoise_history_clamp(g->resolver, 0.0f));
		return SRT_OK;
	}
	if (!(std::isfinite(gamma) && gamma > 0.0f && gamma <= 64.0f))
		return gfail(g, SRT_ERR_INVALID, "srt_group_set_denoise_history_clamp: gamma 0 (off) or finite in (0, 64]");
	if (!g->dn_on || !g->resolver)
		return gfail(g, SRT_ERR_STATE, "srt_group_set_denoise_history_clamp: temporal reprojection is off (srt_group_set_denoise_temporal)");
	SRT_ON_RESOLVER(g, g->resolver, srt_set_denoise_history_clamp(g->resolver, gamma)); // the set-up runs on that handle
	return SRT_OK;
}

int srt_group_last_setup_history_clamp(srt_group *g) { return g && g->resolver && g->resolver->last_setup.clamp ? 1 : 0; }

int srt_group_set_denoise_history_feedback(srt_group *g, int enable) {
	if (!g) return SRT_ERR_INVALID;
	if (!enable) {
		if (g->resolver) SRT_ON_RESOLVER(g, g->resolver, srt_set_denoise_history_feedback(g->resolver, 0));
		return SRT_OK;
	}
	if (!g->dn_on || !g->resolver)
		return gfail(g, SRT_ERR_STATE, "srt_group_set_denoise_history_feedback: temporal reprojection is off (srt_group_set_denoise_temporal)");
	SRT_ON_RESOLVER(g, g->resolver, srt_set_denoise_history_feedback(g->resolver, 1)); // the filter and the commit run on that handle
	return SRT_OK;
}

int srt_group_last_filter_history_feedback(srt_group *g) { return g && g->resolver && g->resolver->last_filter.feedback ? 1 : 0; }

int srt_group_set_denoise_spatial_variance(srt_group *g, uint32_t min_samples) {
	if (!g) return SRT_ERR_INVALID;
	if (min_samples == 0) {
		if (g->resolver) SRT_ON_RESOLVER(g, g->resolver, srt_set_denoise_spatial_variance(g->resolver, 0));
		return SRT_OK;
	}
	if (min_samples > (1u << 20)) return gfail(g, SRT_ERR_INVALID, "srt_group_set_denoise_spatial_variance: min_samples 0..2^20");
	if (!g->dn_on) return gfail(g, SRT_ERR_STATE, "srt_group_set_denoise_spatial_variance: the denoiser is off (srt_group_set_denoise)");
	srt_tracer *r = resolver_of(g);
	if (!r) return SRT_ERR_HIP;
	SRT_ON_RESOLVER(g, r, srt_set_denoise_spatial_variance(r, min_samples)); // the filter runs on that handle
	return SRT_OK;
}

int srt_group_last_filter_spatial_variance(const srt_group *g, int *ran) {
	if (!g || !ran) return SRT_ERR_INVALID;
	*ran = (g->resolver && g->resolver->last_filter.spatial_var) ? 1 : 0;
	return SRT_OK;
}

int srt_group_reset_denoise_history(srt_group *g) {
	if (!g) return SRT_ERR_INVALID;
	drop_history(g);
	return SRT_OK;
}

int srt_group_resolve_denoised(srt_group *g, uint32_t ticks_stopped) {
	if (!g) return SRT_ERR_INVALID;
	if (!g->dn_on) return gfail(g, SRT_ERR_STATE, "srt_group_resolve_denoised: the denoiser is off (srt_group_set_denoise)");
	srt_tracer *r = resolver_of(g);
	if (!r) return SRT_ERR_HIP;
	SRT_ON_RESOLVER(g, r, srt_resolve_denoised(r, ticks_stopped));
	return SRT_OK;
}

int srt_group_read_denoised(srt_group *g, float *rgba_out) {
	if (!g) return SRT_ERR_INVALID;
	if (!rgba_out) return gfail(g, SRT_ERR_INVALID, "srt_group_read_denoised: rgba_out is NULL");
	if (!g->resolver) return gfail(g, SRT_ERR_STATE, "srt_group_read_denoised: no filtered image (srt_group_set_denoise, then render)");
	srt_tracer *r = resolver_of(g);
	SRT_ON_RESOLVER(g, r, srt_read_denoised(r, rgba_out));
	return SRT_OK;
}

int srt_group_read_denoise_inputs(srt_group *g, float *normal_depth, float *albedo_hits, float *moments, uint32_t counts[2]) {
	if (!g) return SRT_ERR_INVALID;
	if (!g->resolver) return gfail(g, SRT_ERR_STATE, "srt_group_read_denoise_inputs: the denoiser was never enabled");
	srt_tracer *r = resolver_of(g);
	SRT_ON_RESOLVER(g, r, srt_read_denoise_inputs(r, normal_depth, albedo_hits, moments, counts)); // as gathered with the last frame
	return SRT_OK;
}

int srt_group_read_denoise_history(srt_group *g, float *colour_count, float *moments, float *guide, srt_render_data *camera, int *valid) {
	if (!g) return SRT_ERR_INVALID;
	if (!g->resolver) return gfail(g, SRT_ERR_STATE, "srt_group_read_denoise_history: temporal reprojection was never enabled (srt_group_set_denoise_temporal)");
	srt_tracer *r = resolver_of(g);
	SRT_ON_RESOLVER(g, r, srt_read_denoise_history(r, colour_count, moments, guide, camera, valid));
	return SRT_OK;
}

// ---- exposure on a group: the first member's state, which the group's resolves on the first device go through ----
int srt_group_set_exposure(srt_group *g, const srt_exposure_params *p) {
	if (!g) return SRT_ERR_INVALID;
	const int rc = srt_set_exposure(g->t[0], p);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_reset_exposure(srt_group *g) {
	if (!g) return SRT_ERR_INVALID;
	const int rc = srt_reset_exposure(g->t[0]);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_read_exposure(srt_group *g, float *log2_exposure, float *exposure, uint32_t hist[256], uint32_t counts[2]) {
	if (!g) return SRT_ERR_INVALID;
	const int rc = srt_read_exposure(g->t[0], log2_exposure, exposure, hist, counts);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_last_resolve_exposed(const srt_group *g, int *exposed) {
	if (!g) return SRT_ERR_INVALID;
	return srt_last_resolve_exposed(g->t[0], exposed);
}

// ---- bloom on a group: the first member's state, as exposure ----
int srt_group_set_bloom(srt_group *g, const srt_bloom_params *p) {
	if (!g) return SRT_ERR_INVALID;
	const int rc = srt_set_bloom(g->t[0], p);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_read_bloom(srt_group *g, int level, float *rgba_out, size_t cap_pixels, int *w, int *h) {
	if (!g) return SRT_ERR_INVALID;
	const int rc = srt_read_bloom(g->t[0], level, rgba_out, cap_pixels, w, h);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_last_resolve_bloomed(const srt_group *g, int *bloomed) {
	if (!g) return SRT_ERR_INVALID;
	return srt_last_resolve_bloomed(g->t[0], bloomed);
}

// ---- the selection overlay on a group: the first member's state and scene; the group's resolves on the first device go through it ----
int srt_group_set_selection(srt_group *g, const srt_selection_params *p, const uint32_t *shapes, size_t n) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	const int rc = srt_set_selection(g->t[0], p, shapes, n);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_read_id_pass(srt_group *g, uint32_t *shape, uint32_t *triangle, int32_t *material, size_t cap_pixels, int *w, int *h) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	const int rc = srt_read_id_pass(g->t[0], shape, triangle, material, cap_pixels, w, h);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_last_resolve_selected(const srt_group *g, int *applied, int *id_pass_ran) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	return srt_last_resolve_selected(g->t[0], applied, id_pass_ran);
}

// ---- noise metering on a group: the single handle's calls on the group's full-frame handle, whose canvas and moments are the
// gathered planes on the first device; the state is the first member's, shared by pointer as the exposure state is ----
namespace {
srt_tracer *noise_resolver(srt_group *g, const char *who) {
	if (!g->dn_on) {
		g->err = std::string(who) + ": the group's denoiser is off: nothing accumulates the moments (srt_group_set_denoise; iterations = 0 is enough)";
		return nullptr;
	}
	return resolver_of(g);
}
} // namespace

int srt_group_set_noise_meter(srt_group *g, const srt_noise_params *p) {
	if (!g) return SRT_ERR_INVALID;
	if (!p || !p->enable) {
		const int rc = srt_set_noise_meter(g->t[0], nullptr);
		return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
	}
	if (srt_noise_check_host(p)) return gfail(g, SRT_ERR_INVALID, "srt_group_set_noise_meter: parameters out of range (srt_noise_check_host)");
	srt_tracer *r = noise_resolver(g, "srt_group_set_noise_meter");
	if (!r) return SRT_ERR_STATE;
	SRT_ON_RESOLVER(g, r, srt_set_noise_meter(r, p));
	return SRT_OK;
}

int srt_group_meter_noise(srt_group *g) {
	if (!g) return SRT_ERR_INVALID;
	srt_tracer *r = noise_resolver(g, "srt_group_meter_noise");
	if (!r) return SRT_ERR_STATE;
	SRT_ON_RESOLVER(g, r, srt_meter_noise(r));
	return SRT_OK;
}

int srt_group_resolve_noise_view(srt_group *g) {
	if (!g) return SRT_ERR_INVALID;
	srt_tracer *r = noise_resolver(g, "srt_group_resolve_noise_view");
	if (!r) return SRT_ERR_STATE;
	SRT_ON_RESOLVER(g, r, srt_resolve_noise_view(r));
	return SRT_OK;
}

int srt_group_poll_noise(srt_group *g, srt_noise_result *result, uint32_t hist[256], int *ready) {
	if (!g) return SRT_ERR_INVALID;
	srt_tracer *r = noise_resolver(g, "srt_group_poll_noise");
	if (!r) return SRT_ERR_STATE;
	SRT_ON_RESOLVER(g, r, srt_poll_noise(r, result, hist, ready));
	return SRT_OK;
}

int srt_group_read_noise(srt_group *g, srt_noise_result *result, uint32_t hist[256]) {
	if (!g) return SRT_ERR_INVALID;
	srt_tracer *r = noise_resolver(g, "srt_group_read_noise");
	if (!r) return SRT_ERR_STATE;
	SRT_ON_RESOLVER(g, r, srt_read_noise(r, result, hist));
	return SRT_OK;
}

int srt_group_read_noise_view(srt_group *g, uint8_t *argb_out) {
	if (!g) return SRT_ERR_INVALID;
	if (!argb_out) return gfail(g, SRT_ERR_INVALID, "srt_group_read_noise_view: argb_out is NULL");
	srt_tracer *r = noise_resolver(g, "srt_group_read_noise_view");
	if (!r) return SRT_ERR_STATE;
	SRT_ON_RESOLVER(g, r, srt_read_argb(r, argb_out));
	return SRT_OK;
}

// ray queries (ray_query.hip) on the first member: every member holds the whole scene, and a query ignores the partition
int srt_group_cast_rays(srt_group *g, const srt_ray *rays, size_t n, uint32_t flags, srt_ray_hit *hits) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	const int rc = srt_cast_rays(g->t[0], rays, n, flags, hits);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_pick(srt_group *g, const srt_render_data *options, const float *xy, size_t n, srt_ray_hit *hits) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	const int rc = srt_pick(g->t[0], options, xy, n, hits);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

// nearest-surface queries (nearest.hip), likewise
int srt_group_nearest_points(srt_group *g, const srt_point_query *queries, size_t n, uint32_t skip_shape, srt_nearest *out) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	const int rc = srt_nearest_points(g->t[0], queries, n, skip_shape, out);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

// occlusion queries (occlusion.hip), likewise
int srt_group_occluded_rays(srt_group *g, const srt_ray *rays, size_t n, uint32_t flags, uint64_t *occluded, uint64_t *invalid) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	const int rc = srt_occluded_rays(g->t[0], rays, n, flags, occluded, invalid);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_occluded_segments(srt_group *g, const srt_segment *segs, size_t n, uint64_t *occluded, uint64_t *invalid) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	const int rc = srt_occluded_segments(g->t[0], segs, n, occluded, invalid);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_segment_rays(srt_group *g, const srt_segment *segs, size_t n, srt_ray *rays_out) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	const int rc = srt_segment_rays(g->t[0], segs, n, rays_out);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

// the ambient-occlusion pass (ao.hip), likewise: planes, rays and view are the first member's
int srt_group_render_ao(srt_group *g, const srt_render_data *options, const srt_ao_params *params) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	const int rc = srt_render_ao(g->t[0], options, params);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_read_ao(srt_group *g, uint32_t *occluded, size_t cap_pixels, int *w, int *h, int *samples) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	const int rc = srt_read_ao(g->t[0], occluded, cap_pixels, w, h, samples);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_ao_rays(srt_group *g, const srt_render_data *options, const srt_ao_params *params, size_t first_pixel, size_t n_pixels, srt_ray *rays_out) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	const int rc = srt_ao_rays(g->t[0], options, params, first_pixel, n_pixels, rays_out);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_resolve_ao_view(srt_group *g) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	const int rc = srt_resolve_ao_view(g->t[0]);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(g->t[0]));
}

int srt_group_read_ao_view(srt_group *g, uint8_t *argb_out) {
	if (!g || g->t.empty()) return SRT_ERR_INVALID;
	if (!argb_out) return gfail(g, SRT_ERR_INVALID, "srt_group_read_ao_view: argb_out is NULL");
	srt_tracer *t = g->t[0]; // (srt_read_argb would stop at the member's own rows: the view is the whole frame)
	hipError_t e = hipSetDevice(t->device);
	if (e == hipSuccess) e = hipMemcpyAsync(argb_out, t->argb.ptr, full_pixels(t) * 4, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
	return e == hipSuccess ? SRT_OK : gfail(g, SRT_ERR_HIP, std::string("srt_group_read_ao_view: ") + hipGetErrorString(e));
}

int srt_group_get_counters(srt_group *g, srt_counters *out) {
	if (!g || !out) return SRT_ERR_INVALID;
	memset(out, 0, sizeof *out);
	for (srt_tracer *t : g->t) {
		srt_counters c;
		const int rc = srt_get_counters(t, &c);
		if (rc != SRT_OK) return gfail(g, rc, srt_last_error(t));
		out->paths += c.paths, out->rays += c.rays, out->sky += c.sky, out->tri_tests += c.tri_tests, out->tri_pass_u += c.tri_pass_u;
		out->nan_pixels += c.nan_pixels, out->watchdog += c.watchdog;
	}
	return SRT_OK;
}

// ---------------------------------------------------------------------------------
// frame pipeline: the interactive loop's render() with frame N's read-back under frame N+1's trace
// ---------------------------------------------------------------------------------
int srt_render_pipelined(srt_tracer *t, const srt_render_data *options, uint32_t ticks_stopped, uint8_t *argb_out, long long *frame_delivered) {
	if (!t) return SRT_ERR_INVALID;
	if (!argb_out) return fail(t, SRT_ERR_INVALID, "srt_render_pipelined: argb_out is NULL");
	SrtCollect *c = collect_of(t);
	if (!c) return fail(t, SRT_ERR_INVALID, "out of host memory");
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t bytes = (size_t)t->owned_rows * t->width * 4;
	if (!c->copy_stream || c->frame_bytes != bytes) {
		if (c->frames_enqueued != c->frames_delivered) return fail(t, SRT_ERR_STATE, "srt_render_pipelined: partition changed with a frame in flight (srt_pipeline_flush first)");
		if (!c->copy_stream) SRT_HIP(t, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
		for (int i = 0; i < 2; i++) {
			if (c->pinned[i]) (void)hipHostFree(c->pinned[i]);
			if (c->dev_argb[i]) (void)hipFree(c->dev_argb[i]);
			c->pinned[i] = c->dev_argb[i] = nullptr;
			SRT_HIP(t, hipHostMalloc(reinterpret_cast<void **>(&c->pinned[i]), bytes ? bytes : 4, hipHostMallocDefault));
			SRT_HIP(t, hipMalloc(reinterpret_cast<void **>(&c->dev_argb[i]), bytes ? bytes : 4));
			if (!c->resolved[i]) SRT_HIP(t, hipEventCreateWithFlags(&c->resolved[i], hipEventDisableTiming));
			if (!c->copied[i]) SRT_HIP(t, hipEventCreateWithFlags(&c->copied[i], hipEventDisableTiming));
		}
		c->frame_bytes = bytes;
	}
	// enqueue frame N: trace + resolve into this frame's own ARGB buffer on the handle's stream, its copy on the copy stream
	const int slot = (int)(c->frames_enqueued & 1);
	int rc = srt_trace_fused(t, options, c->dev_argb[slot], ticks_stopped); // the last reduction resolves into this frame's own image
	if (rc != SRT_OK) return rc;
	if ((rc = srt_exposure_apply_frame(t, ticks_stopped, c->dev_argb[slot])) != SRT_OK) return rc; // exposure.hip: nothing while the feature is off
	if ((rc = srt_selection_apply_frame(t, c->dev_argb[slot])) != SRT_OK) return rc;               // selection.hip: likewise
	SRT_HIP(t, hipEventRecord(c->resolved[slot], t->stream));
	if ((rc = srt_noise_after_resolve(t)) != SRT_OK) return rc; // noise_meter.hip: nothing while the feature is off; the frame's copy does not wait for it
	SRT_HIP(t, hipStreamWaitEvent(c->copy_stream, c->resolved[slot], 0));
	SRT_HIP(t, hipMemcpyAsync(c->pinned[slot], c->dev_argb[slot], bytes, hipMemcpyDeviceToHost, c->copy_stream));
	SRT_HIP(t, hipEventRecord(c->copied[slot], c->copy_stream));
	c->frames_enqueued++;
	// deliver frame N-1 (its trace, resolve and copy ran while the host prepared frame N)
	if (frame_delivered) *frame_delivered = -1;
	if (c->frames_enqueued - c->frames_delivered == 2) {
		const int prev = (int)(c->frames_delivered & 1);
		SRT_HIP(t, hipEventSynchronize(c->copied[prev]));
		memcpy(argb_out, c->pinned[prev], bytes);
		if (frame_delivered) *frame_delivered = c->frames_delivered;
		c->frames_delivered++;
	}
	return SRT_OK;
}

int srt_pipeline_flush(srt_tracer *t, uint8_t *argb_out, long long *frame_delivered) {
	if (!t) return SRT_ERR_INVALID;
	SrtCollect *c = t->collect;
	if (frame_delivered) *frame_delivered = -1;
	if (!c || c->frames_enqueued == c->frames_delivered) return SRT_OK;
	SRT_HIP(t, hipSetDevice(t->device));
	while (c->frames_enqueued != c->frames_delivered) { // at most two; the caller gets the newest
		const int prev = (int)(c->frames_delivered & 1);
		SRT_HIP(t, hipEventSynchronize(c->copied[prev]));
		if (argb_out) memcpy(argb_out, c->pinned[prev], c->frame_bytes);
		if (frame_delivered) *frame_delivered = c->frames_delivered;
		c->frames_delivered++;
	}
	return SRT_OK;
}

} // extern "C"
