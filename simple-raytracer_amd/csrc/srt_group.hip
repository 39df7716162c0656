// srt_group.hip — one process, several GPUs: what `Tracer(width, height, n_devices)` of host/tracer.hpp drives. A group owns a
// handle per device (a row partition of the frame), traces on all of them, collects on the first (srt_collect.hip through
// collect_internal.h: one ncclGather, or device-to-device copies on virtual devices) and resolves there.
//
// Every other srt_group_* call forwards a per-handle call, in one of three ways with a helper each: to every member
// (each_member: what a dispatch reads), to the first member (first_member: state the resolve on the first device reads, and
// queries, which any member could answer), or to the full-frame resolver handle (on_resolver: the denoiser and what reads its
// planes), which a wrapper gets from resolver_of or, for the noise meter, noise_resolver. A new group call is its argument
// checks and one such line, next to its feature's others below.
#include <cmath>
#include <cstring>
#include <new>

#include "collect_internal.h"

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

} // namespace

// ... and for the noise meter, which reads the moments only the group's denoiser accumulates. NULL either way: SRT_ERR_STATE.
// (No part of the ABI, but among the library's dynamic symbols under this name since the meter's group calls came: it stays one.)
extern "C" srt_tracer *noise_resolver(srt_group *g, const char *who) {
	if (!g->dn_on) {
		g->err = std::string(who) + ": the group's denoiser is off: nothing accumulates the moments (srt_group_set_denoise; iterations = 0 is enough)";
		return nullptr;
	}
	return resolver_of(g);
}

namespace {
// a history-dropping call reached the members: the group's history saw the old sky / textures / scene
void drop_history(srt_group *g) {
	if (g->resolver) srt_temporal_drop(g->resolver);
}

// ---- the three ways a group call forwards a per-handle call `fn` (a failure leaves that handle's text in the group) ----
// on every member, up to the first that fails
template <class... P, class... A>
int each_member(srt_group *g, int (*fn)(srt_tracer *, P...), A... args) {
	if (!g) return SRT_ERR_INVALID;
	for (srt_tracer *t : g->t) {
		const int rc = fn(t, args...);
		if (rc != SRT_OK) return gfail(g, rc, srt_last_error(t));
	}
	return SRT_OK;
}

// on one handle of the group's
template <class... P, class... A>
int on_handle(srt_group *g, srt_tracer *t, int (*fn)(srt_tracer *, P...), A... args) {
	const int rc = fn(t, args...);
	return rc == SRT_OK ? SRT_OK : gfail(g, rc, srt_last_error(t));
}

// on the first member
template <class... P, class... A>
int first_member(srt_group *g, int (*fn)(srt_tracer *, P...), A... args) {
	return g ? on_handle(g, g->t[0], fn, args...) : SRT_ERR_INVALID;
}

// on the resolver as resolver_of gave it (NULL: it could not be made)
template <class... P, class... A>
int on_resolver(srt_group *g, srt_tracer *r, int (*fn)(srt_tracer *, P...), A... args) {
	return r ? on_handle(g, r, fn, args...) : SRT_ERR_HIP;
}
// ... and as noise_resolver gives it to `who` (NULL: the denoiser is off, or it could not be made)
template <class... P, class... A>
int on_noise_resolver(srt_group *g, const char *who, int (*fn)(srt_tracer *, P...), A... args) {
	srt_tracer *r = noise_resolver(g, who);
	return r ? on_handle(g, r, fn, args...) : SRT_ERR_STATE;
}

// every member has taken a call that drops a handle's history (as the per-handle call does for its own)
int dropping(srt_group *g, int rc) {
	if (rc == SRT_OK) drop_history(g);
	return rc;
}

// A switch of the filter or the temporal set-up, which live on the resolver. Off reaches the resolver if there is one; on
// demands the denoiser -- `make`: and makes the resolver; else the resolver too, which temporal reprojection has made -- or
// fails with `off_text`.
template <class V>
int resolver_switch(srt_group *g, bool on, bool make, const char *off_text, int (*fn)(srt_tracer *, V), V value) {
	if (!on) return g->resolver ? on_resolver(g, g->resolver, fn, value) : SRT_OK;
	if (!g->dn_on || (!make && !g->resolver)) return gfail(g, SRT_ERR_STATE, off_text);
	return on_resolver(g, make ? resolver_of(g) : g->resolver, fn, value);
}

// ---- trace_and_gather's steps ----
// virtual devices: every member's packed canvas into its slot of the root's buffer, on the member's stream; the root waits for all
int gather_loopback(srt_group *g, size_t count, const srt_tracer *res) {
	srt_tracer *root = g->t[0];
	for (size_t i = 0; i < g->t.size(); i++) {
		srt_tracer *t = g->t[i];
		// (denoiser: a resolve may be enqueued behind the previous frame's unpermute, so the root can still be reading the buffer)
		if (res && i > 0 && hipStreamWaitEvent(t->stream, g->unpermuted, 0) != hipSuccess) return gfail(g, SRT_ERR_HIP, "srt_group: loopback wait");
		if (hipSetDevice(t->device) != hipSuccess ||
		    hipMemcpyAsync(root->collect->gathered.ptr + i * count, t->canvas, count * sizeof(float), hipMemcpyDeviceToDevice, t->stream) != hipSuccess ||
		    hipEventRecord(g->copied[i], t->stream) != hipSuccess)
			return gfail(g, SRT_ERR_HIP, "srt_group: loopback copy of a member's canvas");
	}
	(void)hipSetDevice(root->device);
	for (size_t i = 1; i < g->t.size(); i++) // (the root's own copy is on the root's stream already)
		if (hipStreamWaitEvent(root->stream, g->copied[i], 0) != hipSuccess) return gfail(g, SRT_ERR_HIP, "srt_group: loopback wait");
	return SRT_OK;
}

// the ONE collective of the path: every member's packed canvas over its own xGMI link to the root
int gather_rccl(srt_group *g, size_t count) {
	const int r = rccl_gather_to_first(g->t.data(), (int)g->t.size(), count);
	if (r) return gfail(g, SRT_ERR_HIP, std::string("srt_group: ncclGather: ") + rccl_error_string(r));
	(void)hipSetDevice(g->t[0]->device);
	return SRT_OK;
}

// put the gathered frame back in image order on the root: the canvas alone, or all four planes into the resolver's state
int unpermute_gathered(srt_group *g, srt_tracer *res) {
	srt_tracer *root = g->t[0];
	SrtCollect *rc = root->collect;
	int u = SRT_OK;
	if (!res) u = unpermute_on_root(root, rc);
	else if (launch_unpermute_planes(rc->gathered.ptr, rc->full.ptr, res->dn_nd.ptr, res->dn_ah.ptr, res->dn_mom.ptr, g->width, g->height, (int)g->t.size(),
	                                 g->rpb, root->stream) != hipSuccess)
		u = fail(root, SRT_ERR_HIP, "srt_group: unpermute of the gathered planes");
	else rc->have_full = true;
	return u == SRT_OK ? SRT_OK : gfail(g, u, srt_last_error(root));
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
		if (t && t->collect && t->collect->comm) {
			(void)hipSetDevice(t->device);
			(void)hipStreamSynchronize(t->stream);
			rccl_destroy(t->collect->comm);
			t->collect->comm = nullptr;
		}
	}
	for (srt_tracer *t : g->t) srt_destroy(t);
	delete g;
}

const char *srt_group_last_error(const srt_group *g) { return g ? g->err.c_str() : "srt_group: NULL"; }

// A group that reaches its caller has n_devices >= 1 members: fewer are refused here, and a member that cannot be made takes the
// group with it. No srt_group_* call tests for an empty group.
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
		return fail(nullptr, SRT_ERR_HIP, rccl_error_string(0));
	}
	std::vector<ncclComm_t> comms(n_devices, nullptr);
	const int r = rccl_init_all(comms.data(), n_devices, devs.data());
	if (r) {
		const std::string msg = std::string("srt_group_create: ncclCommInitAll: ") + rccl_error_string(r);
		srt_group_destroy(g);
		return fail(nullptr, SRT_ERR_HIP, msg);
	}
	for (int i = 0; i < n_devices; i++) {
		SrtCollect *c = collect_of(g->t[i]);
		if (!c) {
			// the communicators not yet attached to a handle (i and above) belong to nobody: destroy them here, the attached ones
			// go with their handles in srt_group_destroy
			for (int k = i; k < n_devices; k++)
				if (comms[k]) rccl_destroy(comms[k]);
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
		if (const int rc = on_resolver(g, r, srt_temporal_commit)) return rc;
		r->dn_T = r->dn_P = r->dn_F = 0;
	}
	return each_member(g, srt_clear_canvas);
}

// trace on every device, ONE gather to device 0 of the group, unpermute there; everything asynchronous
int srt_group_trace_and_gather(srt_group *g, const srt_render_data *options) {
	if (!g) return SRT_ERR_INVALID;
	srt_tracer *res = g->dn_on ? resolver_of(g) : nullptr;
	if (g->dn_on && !res) return SRT_ERR_HIP;
	if (const int rc = each_member(g, srt_trace, options)) return rc;
	srt_tracer *root = g->t[0];
	const size_t world = g->t.size(), plane = (size_t)srt_partition_padded_rows(g->height, (int)world, g->rpb) * g->width;
	// floats every rank sends: its padded canvas rows; with the denoiser on its whole gd_pack, the canvas rows and the filter's
	// inputs behind them (52 B per pixel instead of 16) -- still one collective
	const size_t count = res ? gd_slot_floats(plane) : plane * 4;
	if (res) srt_denoise_count(res, *options, g->dn_feature_samples); // the counts of the dispatch every member has just run
	if (hipSetDevice(root->device) != hipSuccess || root->collect->gathered.reserve(count * world) != hipSuccess)
		return gfail(g, SRT_ERR_HIP, "srt_group: gather buffer on the root device");
	if (const int rc = g->loopback ? gather_loopback(g, count, res) : gather_rccl(g, count)) return rc;
	if (const int rc = unpermute_gathered(g, res)) return rc;
	if (g->loopback && res && hipEventRecord(g->unpermuted, root->stream) != hipSuccess) return gfail(g, SRT_ERR_HIP, "srt_group: loopback event");
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
	for (size_t i = 1; i < g->t.size(); i++) // every device has finished its part before the call returns
		if ((rc = on_handle(g, g->t[i], srt_synchronize)) != SRT_OK) return rc;
	return SRT_OK;
}

int srt_group_read_canvas(srt_group *g, float *rgba_out) { return first_member(g, srt_read_gathered, rgba_out, nullptr); }

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

// ---- every member: what a dispatch reads. Sky, textures and per-triangle tables are in the history's pictures, which goes ----
int srt_group_set_skybox(srt_group *g, const float *rgba, int width, int height) { return dropping(g, each_member(g, srt_set_skybox, rgba, width, height)); }
int srt_group_set_textures(srt_group *g, const srt_texture_desc *descs, size_t n) { return dropping(g, each_member(g, srt_set_textures, descs, n)); }
int srt_group_set_material_textures(srt_group *g, const srt_material_texture *bindings, size_t n_materials) {
	return dropping(g, each_member(g, srt_set_material_textures, bindings, n_materials));
}
int srt_group_set_triangle_uvs(srt_group *g, const float *uv, size_t n_triangles) { return dropping(g, each_member(g, srt_set_triangle_uvs, uv, n_triangles)); }
int srt_group_set_triangle_materials(srt_group *g, const int32_t *materials, size_t n_triangles) {
	return dropping(g, each_member(g, srt_set_triangle_materials, materials, n_triangles));
}
int srt_group_set_acceleration(srt_group *g, int mode) { return each_member(g, srt_set_acceleration, mode); }
int srt_group_set_acceleration_refit(srt_group *g, int mode) { return each_member(g, srt_set_acceleration_refit, mode); }
int srt_group_set_acceleration_deform(srt_group *g, int mode, float rebuild_ratio) { return each_member(g, srt_set_acceleration_deform, mode, rebuild_ratio); }
int srt_group_set_acceleration_build(srt_group *g, int mode, uint32_t min_triangles) { return each_member(g, srt_set_acceleration_build, mode, min_triangles); }
int srt_group_set_acceleration_build_order(srt_group *g, int order) { return each_member(g, srt_set_acceleration_build_order, order); }

// ---- the resolver: the denoiser on a group is the per-handle calls on the full-frame handle, the switch carried to the members ----
int srt_group_set_denoise(srt_group *g, const srt_denoise_params *params) {
	if (!g) return SRT_ERR_INVALID;
	if (!params || !params->enable) {
		if (g->resolver)
			if (const int rc = on_resolver(g, g->resolver, srt_set_denoise, nullptr)) return rc; // (drops the history, temporal off)
		if (g->dn_on)
			if (const int rc = each_member(g, srt_denoise_member, 0)) return rc;
		g->dn_on = false;
		return SRT_OK;
	}
	const bool clear = !g->dn_on || params->feature_samples != g->dn_feature_samples;
	// validation, the full-frame buffers, and on `clear` the root's sums and history
	if (const int rc = on_resolver(g, resolver_of(g), srt_set_denoise, params)) return rc;
	if (clear) // canvas rows and sums of every member: zero
		if (const int rc = each_member(g, srt_denoise_member, params->feature_samples)) return rc;
	g->dn_on = true;
	g->dn_feature_samples = params->feature_samples;
	return SRT_OK;
}

int srt_group_set_denoise_temporal(srt_group *g, const srt_temporal_params *params) {
	if (!g) return SRT_ERR_INVALID;
	if ((!params || !params->enable) && !g->resolver) return SRT_OK;
	return on_resolver(g, resolver_of(g), srt_set_denoise_temporal, params);
}

int srt_group_set_denoise_demodulation(srt_group *g, int enable) { // (the filter runs on the resolver)
	if (!g) return SRT_ERR_INVALID;
	return resolver_switch(g, enable != 0, true, "srt_group_set_denoise_demodulation: the denoiser is off (srt_group_set_denoise)", srt_set_denoise_demodulation,
	                       enable ? 1 : 0);
}

int srt_group_set_denoise_history_illumination(srt_group *g, int enable) { // (the set-up runs on the resolver)
	if (!g) return SRT_ERR_INVALID;
	return resolver_switch(g, enable != 0, false, "srt_group_set_denoise_history_illumination: temporal reprojection is off (srt_group_set_denoise_temporal)",
	                       srt_set_denoise_history_illumination, enable ? 1 : 0);
}

int srt_group_set_denoise_history_clamp(srt_group *g, float gamma) { // (likewise)
	if (!g) return SRT_ERR_INVALID;
	if (gamma != 0.0f && !(std::isfinite(gamma) && gamma > 0.0f && gamma <= 64.0f))
		return gfail(g, SRT_ERR_INVALID, "srt_group_set_denoise_history_clamp: gamma 0 (off) or finite in (0, 64]");
	return resolver_switch(g, gamma != 0.0f, false, "srt_group_set_denoise_history_clamp: temporal reprojection is off (srt_group_set_denoise_temporal)",
	                       srt_set_denoise_history_clamp, gamma != 0.0f ? gamma : 0.0f);
}

int srt_group_set_denoise_history_feedback(srt_group *g, int enable) { // (the filter and the commit run on the resolver)
	if (!g) return SRT_ERR_INVALID;
	return resolver_switch(g, enable != 0, false, "srt_group_set_denoise_history_feedback: temporal reprojection is off (srt_group_set_denoise_temporal)",
	                       srt_set_denoise_history_feedback, enable ? 1 : 0);
}

int srt_group_set_denoise_spatial_variance(srt_group *g, uint32_t min_samples) { // (the filter runs on the resolver)
	if (!g) return SRT_ERR_INVALID;
	if (min_samples > (1u << 20)) return gfail(g, SRT_ERR_INVALID, "srt_group_set_denoise_spatial_variance: min_samples 0..2^20");
	return resolver_switch(g, min_samples != 0, true, "srt_group_set_denoise_spatial_variance: the denoiser is off (srt_group_set_denoise)",
	                       srt_set_denoise_spatial_variance, min_samples);
}

int srt_group_last_filter_demodulated(const srt_group *g, int *demodulated) {
	if (!g || !demodulated) return SRT_ERR_INVALID;
	*demodulated = (g->resolver && g->resolver->last_filter.demod) ? 1 : 0;
	return SRT_OK;
}

int srt_group_last_filter_spatial_variance(const srt_group *g, int *ran) {
	if (!g || !ran) return SRT_ERR_INVALID;
	*ran = (g->resolver && g->resolver->last_filter.spatial_var) ? 1 : 0;
	return SRT_OK;
}

// (a flag, not a status: 0 for a NULL group)
int srt_group_last_setup_history_illumination(srt_group *g) { return g && g->resolver && g->resolver->last_setup.illum ? 1 : 0; }
int srt_group_last_setup_history_clamp(srt_group *g) { return g && g->resolver && g->resolver->last_setup.clamp ? 1 : 0; }
int srt_group_last_filter_history_feedback(srt_group *g) { return g && g->resolver && g->resolver->last_filter.feedback ? 1 : 0; }

int srt_group_reset_denoise_history(srt_group *g) {
	if (!g) return SRT_ERR_INVALID;
	drop_history(g);
	return SRT_OK;
}

int srt_group_resolve_denoised(srt_group *g, uint32_t ticks_stopped) {
	if (!g) return SRT_ERR_INVALID;
	if (!g->dn_on) return gfail(g, SRT_ERR_STATE, "srt_group_resolve_denoised: the denoiser is off (srt_group_set_denoise)");
	return on_resolver(g, resolver_of(g), srt_resolve_denoised, ticks_stopped);
}

int srt_group_read_denoised(srt_group *g, float *rgba_out) {
	if (!g) return SRT_ERR_INVALID;
	if (!rgba_out) return gfail(g, SRT_ERR_INVALID, "srt_group_read_denoised: rgba_out is NULL");
	if (!g->resolver) return gfail(g, SRT_ERR_STATE, "srt_group_read_denoised: no filtered image (srt_group_set_denoise, then render)");
	return on_resolver(g, resolver_of(g), srt_read_denoised, rgba_out);
}

int srt_group_read_denoise_inputs(srt_group *g, float *normal_depth, float *albedo_hits, float *moments, uint32_t counts[2]) {
	if (!g) return SRT_ERR_INVALID;
	if (!g->resolver) return gfail(g, SRT_ERR_STATE, "srt_group_read_denoise_inputs: the denoiser was never enabled");
	return on_resolver(g, resolver_of(g), srt_read_denoise_inputs, normal_depth, albedo_hits, moments, counts); // as gathered with the last frame
}

int srt_group_read_denoise_history(srt_group *g, float *colour_count, float *moments, float *guide, srt_render_data *camera, int *valid) {
	if (!g) return SRT_ERR_INVALID;
	if (!g->resolver) return gfail(g, SRT_ERR_STATE, "srt_group_read_denoise_history: temporal reprojection was never enabled (srt_group_set_denoise_temporal)");
	return on_resolver(g, resolver_of(g), srt_read_denoise_history, colour_count, moments, guide, camera, valid);
}

// ---- the resolver again: noise metering is the single handle's calls on the full-frame handle, whose canvas and moments are the
// gathered planes on the first device; the state is the first member's, shared by pointer as the exposure state is ----
int srt_group_set_noise_meter(srt_group *g, const srt_noise_params *p) {
	if (!p || !p->enable) return first_member(g, srt_set_noise_meter, nullptr);
	if (!g) return SRT_ERR_INVALID;
	if (srt_noise_check_host(p)) return gfail(g, SRT_ERR_INVALID, "srt_group_set_noise_meter: parameters out of range (srt_noise_check_host)");
	return on_noise_resolver(g, "srt_group_set_noise_meter", srt_set_noise_meter, p);
}

int srt_group_meter_noise(srt_group *g) { return g ? on_noise_resolver(g, "srt_group_meter_noise", srt_meter_noise) : SRT_ERR_INVALID; }
int srt_group_resolve_noise_view(srt_group *g) { return g ? on_noise_resolver(g, "srt_group_resolve_noise_view", srt_resolve_noise_view) : SRT_ERR_INVALID; }
int srt_group_poll_noise(srt_group *g, srt_noise_result *result, uint32_t hist[256], int *ready) {
	return g ? on_noise_resolver(g, "srt_group_poll_noise", srt_poll_noise, result, hist, ready) : SRT_ERR_INVALID;
}
int srt_group_read_noise(srt_group *g, srt_noise_result *result, uint32_t hist[256]) {
	return g ? on_noise_resolver(g, "srt_group_read_noise", srt_read_noise, result, hist) : SRT_ERR_INVALID;
}
int srt_group_read_noise_view(srt_group *g, uint8_t *argb_out) {
	if (!g) return SRT_ERR_INVALID;
	if (!argb_out) return gfail(g, SRT_ERR_INVALID, "srt_group_read_noise_view: argb_out is NULL");
	return on_noise_resolver(g, "srt_group_read_noise_view", srt_read_argb, argb_out);
}

// ---- the first member: exposure, bloom and the selection overlay are its state, which the group's resolves on the first device go
// through (the resolver shares it by pointer). The three srt_group_last_resolve_* hand the member's code on and leave no text ----
int srt_group_set_exposure(srt_group *g, const srt_exposure_params *p) { return first_member(g, srt_set_exposure, p); }
int srt_group_reset_exposure(srt_group *g) { return first_member(g, srt_reset_exposure); }
int srt_group_read_exposure(srt_group *g, float *log2_exposure, float *exposure, uint32_t hist[256], uint32_t counts[2]) {
	return first_member(g, srt_read_exposure, log2_exposure, exposure, hist, counts);
}
int srt_group_last_resolve_exposed(const srt_group *g, int *exposed) { return g ? srt_last_resolve_exposed(g->t[0], exposed) : SRT_ERR_INVALID; }
int srt_group_set_bloom(srt_group *g, const srt_bloom_params *p) { return first_member(g, srt_set_bloom, p); }
int srt_group_read_bloom(srt_group *g, int level, float *rgba_out, size_t cap_pixels, int *w, int *h) {
	return first_member(g, srt_read_bloom, level, rgba_out, cap_pixels, w, h);
}
int srt_group_last_resolve_bloomed(const srt_group *g, int *bloomed) { return g ? srt_last_resolve_bloomed(g->t[0], bloomed) : SRT_ERR_INVALID; }
int srt_group_set_selection(srt_group *g, const srt_selection_params *p, const uint32_t *shapes, size_t n) { return first_member(g, srt_set_selection, p, shapes, n); }
int srt_group_read_id_pass(srt_group *g, uint32_t *shape, uint32_t *triangle, int32_t *material, size_t cap_pixels, int *w, int *h) {
	return first_member(g, srt_read_id_pass, shape, triangle, material, cap_pixels, w, h);
}
int srt_group_last_resolve_selected(const srt_group *g, int *applied, int *id_pass_ran) {
	return g ? srt_last_resolve_selected(g->t[0], applied, id_pass_ran) : SRT_ERR_INVALID;
}
// area selection (area.hip): the first member holds the group's one ID / selection state and the whole scene
int srt_group_area_coverage(srt_group *g, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t *counts, size_t cap_shapes,
                            srt_area_summary *out) {
	return first_member(g, srt_area_coverage, options, area, vertices, counts, cap_shapes, out);
}
int srt_group_area_triangle_coverage(srt_group *g, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t shape,
                                     uint32_t *counts, size_t cap_triangles, srt_area_summary *out) {
	return first_member(g, srt_area_triangle_coverage, options, area, vertices, shape, counts, cap_triangles, out);
}
int srt_group_select_area(srt_group *g, const srt_render_data *options, const srt_area *area, const int32_t *vertices, int mode, uint32_t min_pixels,
                          size_t *n_selected) {
	return first_member(g, srt_select_area, options, area, vertices, mode, min_pixels, n_selected);
}
int srt_group_read_selection(srt_group *g, uint32_t *shapes, size_t cap, size_t *n) { return first_member(g, srt_read_selection, shapes, cap, n); }
// X-ray area selection (area_through.hip): likewise
int srt_group_area_coverage_through(srt_group *g, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t *counts,
                                    size_t cap_shapes, srt_area_summary *out) {
	return first_member(g, srt_area_coverage_through, options, area, vertices, counts, cap_shapes, out);
}
int srt_group_area_triangle_coverage_through(srt_group *g, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t shape,
                                             uint32_t *counts, size_t cap_triangles, srt_area_summary *out) {
	return first_member(g, srt_area_triangle_coverage_through, options, area, vertices, shape, counts, cap_triangles, out);
}
int srt_group_select_area_through(srt_group *g, const srt_render_data *options, const srt_area *area, const int32_t *vertices, int mode, uint32_t min_pixels,
                                  size_t *n_selected) {
	return first_member(g, srt_select_area_through, options, area, vertices, mode, min_pixels, n_selected);
}
int srt_group_pick_rays(srt_group *g, const srt_render_data *options, const float *xy, size_t n, srt_ray *rays_out) {
	return first_member(g, srt_pick_rays, options, xy, n, rays_out);
}

// ---- the first member again: every member holds the whole scene, and a query ignores the partition. Ray queries (ray_query.hip),
// nearest-surface queries (nearest.hip), occlusion queries (occlusion.hip), the ambient-occlusion pass (ao.hip) ----
int srt_group_cast_rays(srt_group *g, const srt_ray *rays, size_t n, uint32_t flags, srt_ray_hit *hits) { return first_member(g, srt_cast_rays, rays, n, flags, hits); }
int srt_group_cast_rays_multi(srt_group *g, const srt_ray *rays, size_t n, uint32_t k, uint32_t flags, srt_ray_hit *hits, uint32_t *counts) {
	return first_member(g, srt_cast_rays_multi, rays, n, k, flags, hits, counts);
}
int srt_group_pick_through(srt_group *g, const srt_render_data *options, const float *xy, size_t n, uint32_t k, srt_ray_hit *hits, uint32_t *counts) {
	return first_member(g, srt_pick_through, options, xy, n, k, hits, counts);
}
int srt_group_pick(srt_group *g, const srt_render_data *options, const float *xy, size_t n, srt_ray_hit *hits) {
	return first_member(g, srt_pick, options, xy, n, hits);
}
int srt_group_nearest_points(srt_group *g, const srt_point_query *queries, size_t n, uint32_t skip_shape, srt_nearest *out) {
	return first_member(g, srt_nearest_points, queries, n, skip_shape, out);
}
int srt_group_occluded_rays(srt_group *g, const srt_ray *rays, size_t n, uint32_t flags, uint64_t *occluded, uint64_t *invalid) {
	return first_member(g, srt_occluded_rays, rays, n, flags, occluded, invalid);
}
int srt_group_occluded_segments(srt_group *g, const srt_segment *segs, size_t n, uint64_t *occluded, uint64_t *invalid) {
	return first_member(g, srt_occluded_segments, segs, n, occluded, invalid);
}
int srt_group_segment_rays(srt_group *g, const srt_segment *segs, size_t n, srt_ray *rays_out) { return first_member(g, srt_segment_rays, segs, n, rays_out); }
int srt_group_render_ao(srt_group *g, const srt_render_data *options, const srt_ao_params *params) { return first_member(g, srt_render_ao, options, params); }
int srt_group_read_ao(srt_group *g, uint32_t *occluded, size_t cap_pixels, int *w, int *h, int *samples) {
	return first_member(g, srt_read_ao, occluded, cap_pixels, w, h, samples);
}
int srt_group_ao_rays(srt_group *g, const srt_render_data *options, const srt_ao_params *params, size_t first_pixel, size_t n_pixels, srt_ray *rays_out) {
	return first_member(g, srt_ao_rays, options, params, first_pixel, n_pixels, rays_out);
}
int srt_group_resolve_ao_view(srt_group *g) { return first_member(g, srt_resolve_ao_view); }

int srt_group_read_ao_view(srt_group *g, uint8_t *argb_out) {
	if (!g) return SRT_ERR_INVALID;
	if (!argb_out) return gfail(g, SRT_ERR_INVALID, "srt_group_read_ao_view: argb_out is NULL");
	srt_tracer *t = g->t[0]; // (srt_read_argb would stop at the member's own rows: the view is the whole frame)
	hipError_t e = hipSetDevice(t->device);
	if (e == hipSuccess) e = hipMemcpyAsync(argb_out, t->argb.ptr, full_pixels(t) * 4, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
	return e == hipSuccess ? SRT_OK : gfail(g, SRT_ERR_HIP, std::string("srt_group_read_ao_view: ") + hipGetErrorString(e));
}

} // extern "C"
