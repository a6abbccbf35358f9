// amvs_comm.hip -- the native exchange of the C ABI (include/amvs.h).  The only file that sees RCCL.
#include "amvs_ctx.h"

#include <dlfcn.h>
#include <rccl/rccl.h>          // types only: the library is resolved at run time (amvs_comm_*)

#include <cstdlib>
#include <cstring>

using namespace amvs::host;

// ---- native exchange: RCCL through dlopen (no link-time dependency; with a PyTorch-ROCm wheel in the
// process the SONAME librccl.so.1 resolves to the copy torch already loaded) ----
namespace {
struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string why;
};

Rccl &rccl()
{
    static Rccl r = [] {
        Rccl q;
        // AMVS_RCCL_LIB (read once, here): the library to open instead of the default names -- a site with
        // RCCL elsewhere, and the test of the not-found path
        const char *forced = std::getenv("AMVS_RCCL_LIB");
        std::string last;
        if (forced && *forced) {
            q.lib = dlopen(forced, RTLD_NOW | RTLD_GLOBAL);
            if (!q.lib) { const char *e = dlerror(); last = e ? e : ""; }     // (dlerror() clears itself: call it once)
        } else {
            for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
                q.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
                if (q.lib) break;
                const char *e = dlerror();
                last = e ? e : "";
            }
        }
        if (!q.lib) { q.why = "RCCL not found (dlopen " + std::string(forced && *forced ? forced : "librccl.so.1") + "): " + last; return q; }
        q.GetUniqueId = (decltype(q.GetUniqueId))dlsym(q.lib, "ncclGetUniqueId");
        q.CommInitRank = (decltype(q.CommInitRank))dlsym(q.lib, "ncclCommInitRank");
        q.AllGather = (decltype(q.AllGather))dlsym(q.lib, "ncclAllGather");
        q.CommDestroy = (decltype(q.CommDestroy))dlsym(q.lib, "ncclCommDestroy");
        q.GetErrorString = (decltype(q.GetErrorString))dlsym(q.lib, "ncclGetErrorString");
        if (!q.GetUniqueId || !q.CommInitRank || !q.AllGather || !q.CommDestroy || !q.GetErrorString)
            q.why = "RCCL library lacks an expected symbol";
        return q;
    }();
    return r;
}

int rccl_fail(amvs_ctx *c, const char *what, ncclResult_t e)
{
    return fail(c, AMVS_EHIP, std::string(what) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(e) : "RCCL error"));
}
}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int amvs_comm_unique_id(uint8_t id_out[AMVS_COMM_ID_BYTES])
{
    static_assert(sizeof(ncclUniqueId) == AMVS_COMM_ID_BYTES, "ncclUniqueId size");
    if (!id_out) return fail(nullptr, AMVS_EINVAL, "NULL id");
    if (!rccl().why.empty()) return fail(nullptr, AMVS_EUNSUPPORTED, rccl().why);
    ncclUniqueId id;
    const ncclResult_t e = rccl().GetUniqueId(&id);
    if (e != ncclSuccess) return rccl_fail(nullptr, "ncclGetUniqueId", e);
    std::memcpy(id_out, &id, AMVS_COMM_ID_BYTES);
    return AMVS_OK;
}

int amvs_comm_init(amvs_ctx *c, int rank, int world, const uint8_t id_in[AMVS_COMM_ID_BYTES])
{
    if (!c) return AMVS_EINVAL;
    if (!id_in || world < 1 || rank < 0 || rank >= world) return fail(c, AMVS_EINVAL, "bad rank / world / id");
    if (!rccl().why.empty()) return fail(c, AMVS_EUNSUPPORTED, rccl().why);
    int rc = bind_device(c);
    if (rc) return rc;
    if ((rc = amvs_comm_destroy(c))) return rc;
    ncclUniqueId id;
    std::memcpy(&id, id_in, AMVS_COMM_ID_BYTES);
    const ncclResult_t e = rccl().CommInitRank(&c->comm, world, id, rank);
    if (e != ncclSuccess) { c->comm = nullptr; return rccl_fail(c, "ncclCommInitRank", e); }
    c->comm_rank = rank; c->comm_world = world;
    return AMVS_OK;
}

int amvs_allgather_maps(amvs_ctx *c, const void *local_dev, void *full_dev, int64_t floats_per_rank)
{
    if (!c) return AMVS_EINVAL;
    if (!c->comm) return fail(c, AMVS_EINVAL, "no communicator (amvs_comm_init)");
    if (!local_dev || !full_dev || floats_per_rank < 1) return fail(c, AMVS_EINVAL, "bad buffers / count");
    int rc = bind_device(c);
    if (rc) return rc;
    const ncclResult_t e = rccl().AllGather(local_dev, full_dev, (size_t)floats_per_rank, ncclFloat, c->comm, c->stream);
    if (e != ncclSuccess) return rccl_fail(c, "ncclAllGather", e);
    return AMVS_OK;
}

int amvs_comm_destroy(amvs_ctx *c)
{
    if (!c) return AMVS_EINVAL;
    if (c->comm) {
        (void)hipSetDevice(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        const ncclResult_t e = rccl().CommDestroy(c->comm);
        c->comm = nullptr; c->comm_world = 0;
        if (e != ncclSuccess) return rccl_fail(c, "ncclCommDestroy", e);
    }
    return AMVS_OK;
}

}  // extern "C"
#pragma GCC visibility pop
