// srt_collect.hip — collecting the row partition of a multi-GPU frame on one GPU: ONE ncclGather (RCCL over xGMI) of the
// packed per-rank canvases, then an unpermute kernel on the root. Here: RCCL itself, a handle's collection state, the
// unpermute kernels and their launchers, and the path of one process per GPU (srt_comm_*, srt_gather). One process driving
// several GPUs (srt_group_*) is srt_group.hip, which reaches this unit through collect_internal.h. New work: the reference is
// single-device (/root/reference/src/tracer.cpp:13).
//
// RCCL is loaded with dlopen at first use, so libsrt_hip.so has no link-time dependency on it and a
// single-GPU user never touches it.
#include <dlfcn.h>

#include <cstring>
#include <new>

#include "collect_internal.h"

// ---------------------------------------------------------------------------------
// RCCL entry points (signatures of /opt/rocm/include/rccl/rccl.h)
// ---------------------------------------------------------------------------------
namespace {
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

#define SRT_NCCL(t, call)                                                                                        \
	do {                                                                                                         \
		int r_ = (call);                                                                                         \
		if (r_ != kNcclSuccess) return fail((t), SRT_ERR_HIP, std::string(#call) + ": " + rccl().GetErrorString(r_)); \
	} while (0)
} // namespace

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

int rccl_init_all(ncclComm_t *comms, int n, const int *devices) { return rccl().CommInitAll(comms, n, devices); }

void rccl_destroy(ncclComm_t comm) {
	if (rccl().lib) (void)rccl().CommDestroy(comm);
}

int rccl_gather_to_first(srt_tracer *const *members, int world, size_t count) {
	int r = rccl().GroupStart();
	for (int i = 0; i < world && r == kNcclSuccess; i++) {
		srt_tracer *t = members[i];
		(void)hipSetDevice(t->device);
		r = rccl().Gather(t->canvas, i == 0 ? t->collect->gathered.ptr : nullptr, count, kNcclFloat, 0, t->collect->comm, t->stream);
	}
	const int r2 = rccl().GroupEnd();
	return r != kNcclSuccess ? r : r2;
}

const char *rccl_error_string(int code) { return code == kNcclSuccess ? rccl().error.c_str() : rccl().GetErrorString(code); }

SrtCollect *collect_of(srt_tracer *t) {
	if (!t->collect) t->collect = new (std::nothrow) SrtCollect();
	return t->collect;
}

namespace {
// one thread per pixel of the frame up to a cap, a grid-stride loop beyond it: the geometry of both unpermute kernels
unsigned unpermute_blocks(int width, int height) {
	const size_t blocks = ((size_t)width * height + 255) / 256;
	return blocks > 8192 ? 8192u : (unsigned)blocks;
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

} // namespace

hipError_t launch_unpermute(const float *gathered, float *image, int width, int height, int world, int rpb, hipStream_t stream) {
	hipLaunchKernelGGL(srt_unpermute_kernel, dim3(unpermute_blocks(width, height)), dim3(256), 0, stream, reinterpret_cast<const float4 *>(gathered),
	                   reinterpret_cast<float4 *>(image), width, height, world, rpb, srt_partition_padded_rows(height, world, rpb));
	return hipGetLastError();
}

hipError_t launch_unpermute_planes(const float *gathered, float *canvas, float *nd, float *ah, float *mom, int width, int height, int world, int rpb,
                                   hipStream_t stream) {
	const int padded = srt_partition_padded_rows(height, world, rpb);
	hipLaunchKernelGGL(srt_unpermute_planes_kernel, dim3(unpermute_blocks(width, height)), dim3(256), 0, stream, gathered,
	                   reinterpret_cast<float4 *>(canvas), reinterpret_cast<float4 *>(nd), reinterpret_cast<float4 *>(ah), mom, width, height, world, rpb,
	                   padded, gd_slot_floats((size_t)padded * width));
	return hipGetLastError();
}

int unpermute_on_root(srt_tracer *t, SrtCollect *c) {
	const size_t n = (size_t)t->width * t->height;
	SRT_HIP(t, c->full.reserve(n * 4));
	if (const hipError_t e = launch_unpermute(c->gathered.ptr, c->full.ptr, t->width, t->height, t->world, t->rows_per_block, t->stream))
		return fail(t, SRT_ERR_HIP, std::string("hipGetLastError(): ") + hipGetErrorString(e)); // (the text SRT_HIP gave it at the launch)
	c->have_full = true;
	return SRT_OK;
}

void srt_collect_release(srt_tracer *t) {
	SrtCollect *c = t->collect;
	if (!c) return;
	if (c->comm && c->comm_owned) rccl_destroy(c->comm);
	c->gathered.release();
	c->full.release();
	c->full_argb.release();
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
	if (launch_unpermute(static_cast<const float *>(gathered), static_cast<float *>(image), width, height, world, rows_per_block, nullptr) != hipSuccess ||
	    hipDeviceSynchronize() != hipSuccess)
		return SRT_ERR_HIP;
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
	                            static_cast<float *>(albedo_hits), static_cast<float *>(moments), width, height, world, rows_per_block, nullptr) != hipSuccess ||
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
