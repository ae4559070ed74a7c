// cabi_comm.hip - the communicator entries of include/dpfhe.h over RCCL.
#include <dlfcn.h>

#include <cstring>
#include <new>

#include "cabi.h"

// ------------------------------------------------------------------------------------------------
// (e) RCCL all-gather.  librccl is opened lazily so that single-GPU users never depend on it.
// ------------------------------------------------------------------------------------------------
namespace {
struct NcclUniqueId { char internal[128]; };
typedef void* ncclComm_t;
struct Rccl {
    void* h = nullptr;
    int (*GetUniqueId)(NcclUniqueId*) = nullptr;
    int (*CommInitRank)(ncclComm_t*, int, NcclUniqueId, int) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, ncclComm_t, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok = false;
};
Rccl& rccl() {
    static Rccl r = [] {
        Rccl x;
        x.h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!x.h) x.h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!x.h) return x;
        x.GetUniqueId = reinterpret_cast<decltype(x.GetUniqueId)>(dlsym(x.h, "ncclGetUniqueId"));
        x.CommInitRank = reinterpret_cast<decltype(x.CommInitRank)>(dlsym(x.h, "ncclCommInitRank"));
        x.CommDestroy = reinterpret_cast<decltype(x.CommDestroy)>(dlsym(x.h, "ncclCommDestroy"));
        x.AllGather = reinterpret_cast<decltype(x.AllGather)>(dlsym(x.h, "ncclAllGather"));
        x.AllReduce = reinterpret_cast<decltype(x.AllReduce)>(dlsym(x.h, "ncclAllReduce"));
        x.GetErrorString = reinterpret_cast<decltype(x.GetErrorString)>(dlsym(x.h, "ncclGetErrorString"));
        x.ok = x.GetUniqueId && x.CommInitRank && x.CommDestroy && x.AllGather && x.AllReduce;
        return x;
    }();
    return r;
}
const int kNcclUint64 = 5;  // ncclUint64 in rccl.h's ncclDataType_t
int rccl_fail(const char* what, int rc) {
    Rccl& r = rccl();
    return fail(DPFHE_RUNTIME_ERROR, what, r.GetErrorString ? r.GetErrorString(rc) : "rccl error");
}
}  // namespace

struct dpfhe_comm {
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1, device = 0;
};

extern "C" int dpfhe_comm_unique_id(uint8_t out_id[128]) {
    if (!out_id) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_comm_unique_id", "null argument");
    Rccl& r = rccl();
    if (!r.ok) return fail(DPFHE_RUNTIME_ERROR, "dpfhe_comm_unique_id", "librccl.so.1 not loadable");
    NcclUniqueId id;
    int rc = r.GetUniqueId(&id);
    if (rc) return rccl_fail("ncclGetUniqueId", rc);
    std::memcpy(out_id, id.internal, 128);
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_comm_create(dpfhe_comm** out, const uint8_t id[128], int rank, int world_size, int device_id) {
    if (!out || !id || world_size < 1 || rank < 0 || rank >= world_size) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_comm_create", "bad argument");
    Rccl& r = rccl();
    if (!r.ok) return fail(DPFHE_RUNTIME_ERROR, "dpfhe_comm_create", "librccl.so.1 not loadable");
    HIP_TRY(hipSetDevice(device_id));
    dpfhe_comm* c = new (std::nothrow) dpfhe_comm;
    if (!c) return fail(DPFHE_OUT_OF_MEMORY, "dpfhe_comm_create", "host allocation");
    c->rank = rank; c->world = world_size; c->device = device_id;
    NcclUniqueId uid;
    std::memcpy(uid.internal, id, 128);
    int rc = r.CommInitRank(&c->comm, world_size, uid, rank);
    if (rc) { delete c; return rccl_fail("ncclCommInitRank", rc); }
    *out = c;
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_comm_destroy(dpfhe_comm* c) {
    if (!c) return DPFHE_SUCCESS;
    if (c->comm) (void)rccl().CommDestroy(c->comm);
    delete c;
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_comm_allgather(dpfhe_comm* c, uint64_t* d_recv, const uint64_t* d_send, size_t words_per_rank, void* stream) {
    if (!c || !d_recv || !d_send) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_comm_allgather", "null argument");
    if (words_per_rank == 0) return DPFHE_SUCCESS;
    DeviceGuard guard(c->device);
    if (guard.err != hipSuccess) return fail(DPFHE_DEVICE_ERROR, "dpfhe_comm_allgather", hipGetErrorString(guard.err));
    int rc = rccl().AllGather(d_send, d_recv, words_per_rank, kNcclUint64, c->comm, static_cast<hipStream_t>(stream));
    if (rc) return rccl_fail("ncclAllGather", rc);
    return DPFHE_SUCCESS;
}

// SURVEY.md section 8(e)'s alternative to the all-gather, ready for the first multi-GPU lease: ncclAllReduce(ncclUint64, ncclSum) of the ranks' partial
// ciphertexts in place, then ONE mod-q pass - safe because world_size * q < 2^64 for world_size <= 15 (q < 2^60).  Same words as all-gather + local sum.
extern "C" int dpfhe_comm_allreduce_sum(dpfhe_comm* c, dpfhe_ctx* ctx, uint64_t* d_io, size_t n_rns_polys, void* stream) {
    if (!c || !ctx || !d_io) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_comm_allreduce_sum", "null argument");
    if (c->world > 15) return fail(DPFHE_INVALID_STATE, "dpfhe_comm_allreduce_sum", "the lazy sum of more than 15 residues below 2^60 does not fit 64 bits");
    if (c->device != ctx->device) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_comm_allreduce_sum", "communicator and context live on different devices");
    if (n_rns_polys == 0) return DPFHE_SUCCESS;
    {
        DeviceGuard guard(c->device);
        if (guard.err != hipSuccess) return fail(DPFHE_DEVICE_ERROR, "dpfhe_comm_allreduce_sum", hipGetErrorString(guard.err));
        const size_t words = n_rns_polys * ctx->n_limbs << ctx->log2n;
        const int ncclSum = 0;   // rccl.h ncclRedOp_t
        int rc = rccl().AllReduce(d_io, d_io, words, kNcclUint64, ncclSum, c->comm, static_cast<hipStream_t>(stream));
        if (rc) return rccl_fail("ncclAllReduce", rc);
    }
    return dpfhe_canonicalize_sum(ctx, d_io, n_rns_polys, stream);
}
