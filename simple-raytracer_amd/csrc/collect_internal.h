// collect_internal.h — what the device group (srt_group.hip) needs of collection (srt_collect.hip): a handle's collection
// state, the unpermute launchers and RCCL behind plain functions (the dlopen'd table itself stays in srt_collect.hip).
// Not part of the public ABI, and not exported: the library's dynamic symbols are the public ones and srt_internal.h's.
#ifndef SRT_COLLECT_INTERNAL_H
#define SRT_COLLECT_INTERNAL_H

#include "srt_internal.h"

#pragma GCC visibility push(hidden)
typedef struct ncclComm *ncclComm_t;

struct SrtCollect {
	ncclComm_t comm = nullptr;
	bool comm_owned = false; // created by srt_comm_init (else by a group's ncclCommInitAll)
	int comm_rank = -1, comm_world = 0;
	DevBuf<float> gathered; // root: world x padded_rows x width float4, rank-major
	DevBuf<float> full;     // root: height x width float4, the unpermuted image
	DevBuf<uint8_t> full_argb;
	bool have_full = false;
};
SrtCollect *collect_of(srt_tracer *t); // made at first use; NULL: out of host memory

// The launch of each unpermute kernel, THE place its geometry is written: gathered (world slots, rank-major) -> image order, on
// `stream`; hipGetLastError() behind the launch. The planes' form takes slots of gd_slot_floats() floats.
hipError_t launch_unpermute(const float *gathered, float *image, int width, int height, int world, int rpb, hipStream_t stream);
hipError_t launch_unpermute_planes(const float *gathered, float *canvas, float *nd, float *ah, float *mom, int width, int height, int world, int rpb,
                                   hipStream_t stream);
// ... and the handle's path around the first: c->gathered -> c->full (grown to the frame) on t's stream, sets have_full
int unpermute_on_root(srt_tracer *t, SrtCollect *c);

// RCCL, loaded at first use. A code is ncclResult_t's: 0 = success.
bool rccl_load();                                                       // false: rccl_error_string(0) says why
int rccl_init_all(ncclComm_t *comms, int n, const int *devices);        // ncclCommInitAll
void rccl_destroy(ncclComm_t comm);                                     // ncclCommDestroy
int rccl_gather_to_first(srt_tracer *const *members, int world, size_t count); // one ncclGroupStart / End around a ncclGather of `count` floats per member, each on its own device and stream, into members[0]'s `gathered`
const char *rccl_error_string(int code);                                // ncclGetErrorString; 0: the loader's own text
#pragma GCC visibility pop

#endif
