// libgt4py_amd.so -- extern "C" entry points declared in include/gt4py_amd.h.
//
// Each stencil entry replaces the pybind11 `run_computation` the reference generates per stencil
// (/root/reference/src/gt4py/cartesian/backend/gtc_common.py:65-103): validate the fields against
// the domain, shift pointers by the origins (gtc_common.py:48 `sid::shift_sid_origin`), launch the
// hand-written gfx950 kernel on the caller's stream.
#include <chrono>
#include <cstring>

#include "comm.hip.h"
#include "common.hip.h"
#include "halo.hip.h"
#include "halo_fill.hip.h"
#include "field_stats.hip.h"
#include "level_stats.hip.h"
#include "line_stats.hip.h"
#include "field_copy.hip.h"
#include "vertical_remap.hip.h"
#include "vertical_interp.hip.h"
#include "horizontal_interp.hip.h"
#include "departure_interp.hip.h"
#include "point_sample.hip.h"
#include "horizontal_remap.hip.h"
#include "line_solve.hip.h"
#include "line_scan.hip.h"
#include "line_find.hip.h"
#include "field_histogram.hip.h"
#include "line_filter.hip.h"
#include "memprobe.hip.h"
#include "hdiff.hip.h"
#include "hdiff_ring.hip.h"
#include "lap5.hip.h"
#include "lap5_push.hip.h"
#include "lap5_ring.hip.h"
#include "lap5_edge.hip.h"
#include "rtc.hip.h"
#include "tridiag.hip.h"
#include "dist_step.hip.h"

namespace {

inline double now_seconds() {
    using clock = std::chrono::steady_clock;
    return std::chrono::duration<double>(clock::now().time_since_epoch()).count();
}

// Brackets one entry point: host timestamps of the (asynchronous) call and, from a hipEvent pair on the launch
// stream, the time its kernels spent on the device.  Costs nothing when the caller passes no exec_info.
struct Timer {
    gt4mi_exec_info* info;
    hipStream_t stream;
    Timer(gt4mi_exec_info* i, void* s) : info(i), stream(static_cast<hipStream_t>(s)) {
        if (!info) return;
        info->run_cpp_start_time = now_seconds();
        info->run_hip_start_time = info->run_hip_end_time = 0.0;
        if (events_ready()) (void)hipEventRecord(events()[0], stream);
    }
    ~Timer() {
        if (!info) return;
        info->run_cpp_end_time = now_seconds();
        if (!events_ready() || hipEventRecord(events()[1], stream) != hipSuccess ||
            hipEventSynchronize(events()[1]) != hipSuccess) {
            (void)hipGetLastError();
            return;
        }
        float ms = 0.0f;
        const double end = now_seconds();
        if (hipEventElapsedTime(&ms, events()[0], events()[1]) == hipSuccess) {
            info->run_hip_end_time = end;
            info->run_hip_start_time = end - (double)ms * 1e-3;
        }
    }
    static hipEvent_t* events() {
        static thread_local hipEvent_t ev[2] = {nullptr, nullptr};
        return ev;
    }
    static bool events_ready() {
        hipEvent_t* ev = events();
        if (ev[0] == nullptr)
            if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess) {
                ev[0] = ev[1] = nullptr;
                (void)hipGetLastError();
            }
        return ev[0] != nullptr;
    }
};

}  // namespace

extern "C" {

int gt4mi_abi_version(void) { return GT4MI_ABI_VERSION; }

const char* gt4mi_last_error(void) { return gt4mi::error_buffer(); }

int gt4mi_device_info(char* buf, size_t buflen) {
    if (buf == nullptr || buflen == 0) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "device_info: null buffer");
    int dev = 0;
    GT4MI_HIP_CHECK(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    GT4MI_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    snprintf(buf, buflen, "device=%d name=%s arch=%s cus=%d clock_mhz=%d mem_gib=%.1f", dev, prop.name,
             prop.gcnArchName, prop.multiProcessorCount, prop.clockRate / 1000,
             (double)prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0));
    return GT4MI_OK;
}

int gt4mi_stream_sync(void* stream) {
    GT4MI_HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return GT4MI_OK;
}

int gt4mi_lap5_f64(const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* out, int variant,
                   int flags, void* stream, gt4mi_exec_info* info) {
    (void)flags;
    Timer t(info, stream);
    return gt4mi::lap5_run<double, double>(domain, inp, out, variant, static_cast<hipStream_t>(stream));
}

int gt4mi_lap5_f32(const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* out, int variant,
                   int flags, void* stream, gt4mi_exec_info* info) {
    Timer t(info, stream);
    if (flags & GT4MI_LAP_LITERAL_F32)
        return gt4mi::lap5_run<float, float>(domain, inp, out, variant, static_cast<hipStream_t>(stream));
    return gt4mi::lap5_run<float, double>(domain, inp, out, variant, static_cast<hipStream_t>(stream));
}

int gt4mi_hdiff_f64(const int64_t domain[3], const gt4mi_field* in_field, const gt4mi_field* out_field,
                    const gt4mi_field* coeff, double coeff_scalar, int flags, void* stream,
                    gt4mi_exec_info* info) {
    Timer t(info, stream);
    return gt4mi::hdiff_run<double>(domain, in_field, out_field, coeff, coeff_scalar, flags,
                                    static_cast<hipStream_t>(stream));
}

int gt4mi_hdiff_f32(const int64_t domain[3], const gt4mi_field* in_field, const gt4mi_field* out_field,
                    const gt4mi_field* coeff, double coeff_scalar, int flags, void* stream,
                    gt4mi_exec_info* info) {
    Timer t(info, stream);
    return gt4mi::hdiff_run<float>(domain, in_field, out_field, coeff, coeff_scalar, flags,
                                   static_cast<hipStream_t>(stream));
}

int gt4mi_hdiff_ring_f64(const int64_t domain[3], const gt4mi_field* in_field, const gt4mi_field* out_field,
                         const gt4mi_field* coeff, double coeff_scalar, int flags, const int widths[4], void* stream,
                         gt4mi_exec_info* info) {
    Timer t(info, stream);
    return gt4mi::hdiff_ring_run<double>(domain, in_field, out_field, coeff, coeff_scalar, flags, widths,
                                         static_cast<hipStream_t>(stream));
}

int gt4mi_hdiff_ring_f32(const int64_t domain[3], const gt4mi_field* in_field, const gt4mi_field* out_field,
                         const gt4mi_field* coeff, double coeff_scalar, int flags, const int widths[4], void* stream,
                         gt4mi_exec_info* info) {
    Timer t(info, stream);
    return gt4mi::hdiff_ring_run<float>(domain, in_field, out_field, coeff, coeff_scalar, flags, widths,
                                        static_cast<hipStream_t>(stream));
}

int gt4mi_lap5_ring_f64(const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* out, int variant, int flags,
                        const int outer[4], const int inner[4], void* stream, gt4mi_exec_info* info) {
    (void)flags;
    Timer t(info, stream);
    return gt4mi::lap5_ring_run<double, double>(domain, inp, out, variant, outer, inner, static_cast<hipStream_t>(stream));
}

int gt4mi_lap5_ring_f32(const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* out, int variant, int flags,
                        const int outer[4], const int inner[4], void* stream, gt4mi_exec_info* info) {
    Timer t(info, stream);
    if (flags & GT4MI_LAP_LITERAL_F32)
        return gt4mi::lap5_ring_run<float, float>(domain, inp, out, variant, outer, inner, static_cast<hipStream_t>(stream));
    return gt4mi::lap5_ring_run<float, double>(domain, inp, out, variant, outer, inner, static_cast<hipStream_t>(stream));
}

int gt4mi_tridiag_f64(const int64_t domain[3], const gt4mi_field* inf, const gt4mi_field* diag,
                      const gt4mi_field* sup, const gt4mi_field* rhs, const gt4mi_field* out, void* stream,
                      gt4mi_exec_info* info) {
    Timer t(info, stream);
    return gt4mi::tridiag_run<double>(domain, inf, diag, sup, rhs, out, static_cast<hipStream_t>(stream));
}

int gt4mi_tridiag_f32(const int64_t domain[3], const gt4mi_field* inf, const gt4mi_field* diag,
                      const gt4mi_field* sup, const gt4mi_field* rhs, const gt4mi_field* out, void* stream,
                      gt4mi_exec_info* info) {
    Timer t(info, stream);
    return gt4mi::tridiag_run<float>(domain, inf, diag, sup, rhs, out, static_cast<hipStream_t>(stream));
}

int gt4mi_halo_pack(const gt4mi_field* field, const int64_t lo[3], const int64_t extent[3], void* buffer,
                    int elem_size, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (elem_size == 8) return gt4mi::halo_copy<uint64_t, true>(field, lo, extent, buffer, s);
    if (elem_size == 4) return gt4mi::halo_copy<uint32_t, true>(field, lo, extent, buffer, s);
    return gt4mi::fail(GT4MI_ERR_UNSUPPORTED, "halo_pack: element size %d", elem_size);
}

int gt4mi_halo_unpack(const gt4mi_field* field, const int64_t lo[3], const int64_t extent[3],
                      const void* buffer, int elem_size, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    void* b = const_cast<void*>(buffer);
    if (elem_size == 8) return gt4mi::halo_copy<uint64_t, false>(field, lo, extent, b, s);
    if (elem_size == 4) return gt4mi::halo_copy<uint32_t, false>(field, lo, extent, b, s);
    return gt4mi::fail(GT4MI_ERR_UNSUPPORTED, "halo_unpack: element size %d", elem_size);
}

int gt4mi_halo_fill(const gt4mi_field* fields, int nfields, const int64_t domain[3], const int64_t halo[4], int mode_i,
                    int mode_j, int sides, const void* value, int elem_size, void* stream, int* launches) {
    return gt4mi::halo_fill(fields, nfields, domain, halo, mode_i, mode_j, sides, value, elem_size,
                            static_cast<hipStream_t>(stream), launches);
}

int gt4mi_field_stats(const gt4mi_field* fields, const gt4mi_field* others, int nfields, const int64_t domain[3], int elem_size,
                      void* workspace, int64_t workspace_bytes, double* result, int flags, void* stream,
                      int64_t* workspace_needed, int* launches) {
    return gt4mi::field_stats(fields, others, nfields, domain, elem_size, workspace, workspace_bytes, result, flags,
                              static_cast<hipStream_t>(stream), workspace_needed, launches);
}

int gt4mi_level_stats(const gt4mi_field* fields, const gt4mi_field* others, int nfields, const int64_t domain[3], int elem_size,
                      void* workspace, int64_t workspace_bytes, double* result, int flags, void* stream, int64_t* workspace_needed,
                      int* launches) {
    return gt4mi::level_stats(fields, others, nfields, domain, elem_size, workspace, workspace_bytes, result, flags,
                              static_cast<hipStream_t>(stream), workspace_needed, launches);
}

int gt4mi_line_stats(const gt4mi_field* fields, const gt4mi_field* others, int nfields, const int64_t domain[3], int axis, int elem_size,
                     void* workspace, int64_t workspace_bytes, double* result, int flags, void* stream, int64_t* workspace_needed,
                     int* launches, int* path) {
    return gt4mi::line_stats(fields, others, nfields, domain, axis, elem_size, workspace, workspace_bytes, result, flags,
                             static_cast<hipStream_t>(stream), workspace_needed, launches, path);
}

int gt4mi_field_copy(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const int64_t extent[3], int dst_elem_size,
                     int src_elem_size, int flags, void* stream, int* paths, int* launches) {
    return gt4mi::field_copy(dst, src, nfields, extent, dst_elem_size, src_elem_size, flags, static_cast<hipStream_t>(stream), paths,
                             launches);
}

int gt4mi_vertical_remap(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* src_edges,
                         const gt4mi_field* dst_edges, const int64_t extent_ij[2], int64_t ns, int64_t nd, int elem_size,
                         int edge_elem_size, int method, int flags, void* stream, int* launches) {
    return gt4mi::vertical_remap(dst, src, nfields, src_edges, dst_edges, extent_ij, ns, nd, elem_size, edge_elem_size, method, flags,
                                 static_cast<hipStream_t>(stream), launches);
}

int gt4mi_vertical_interp(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* src_coord,
                          const gt4mi_field* dst_coord, const int64_t extent_ij[2], int64_t ns, int64_t nd, int elem_size,
                          int coord_elem_size, int method, int outside, double fill_value, int flags, void* stream, int* launches) {
    return gt4mi::vertical_interp(dst, src, nfields, src_coord, dst_coord, extent_ij, ns, nd, elem_size, coord_elem_size, method, outside,
                                  fill_value, flags, static_cast<hipStream_t>(stream), launches);
}

int gt4mi_horizontal_interp(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* pos_i,
                            const gt4mi_field* pos_j, const int64_t extent[3], const int64_t reach[4], int elem_size,
                            int pos_elem_size, int method, int flags, void* stream, int* launches) {
    return gt4mi::horizontal_interp(dst, src, nfields, pos_i, pos_j, extent, reach, elem_size, pos_elem_size, method, flags,
                                    static_cast<hipStream_t>(stream), launches);
}

int gt4mi_departure_interp(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* pos_i,
                           const gt4mi_field* pos_j, const gt4mi_field* pos_k, const int64_t extent[3], const int64_t reach[4],
                           int elem_size, int pos_elem_size, int method, int flags, void* stream, int* launches) {
    return gt4mi::departure_interp(dst, src, nfields, pos_i, pos_j, pos_k, extent, reach, elem_size, pos_elem_size, method, flags,
                                   static_cast<hipStream_t>(stream), launches);
}

int gt4mi_point_sample(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* pos_i, const gt4mi_field* pos_j,
                       const gt4mi_field* pos_k, int64_t npoints, const int64_t extent[3], const int64_t reach[4], int elem_size,
                       int pos_elem_size, int method, int flags, double fill_value, void* stream, int* launches) {
    return gt4mi::point_sample(dst, src, nfields, pos_i, pos_j, pos_k, npoints, extent, reach, elem_size, pos_elem_size, method, flags,
                               fill_value, static_cast<hipStream_t>(stream), launches);
}

int gt4mi_overlap_table(const double* src_edges, int ns, const double* dst_edges, int nd, int32_t* ptr, int32_t* cell, double* w,
                        double* h, double* c, double* den, int capacity, int* nnz) {
    return gt4mi::overlap_table(src_edges, ns, dst_edges, nd, ptr, cell, w, h, c, den, capacity, nnz);
}

int gt4mi_horizontal_remap(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_overlap_axis* axis_i,
                           const gt4mi_overlap_axis* axis_j, int64_t nk, int elem_size, int method, int flags, void* stream,
                           int* launches) {
    return gt4mi::horizontal_remap(dst, src, nfields, axis_i, axis_j, nk, elem_size, method, flags, static_cast<hipStream_t>(stream),
                                   launches);
}

int gt4mi_line_solve(const gt4mi_field* out, const gt4mi_field* rhs, int nfields, const gt4mi_field* lower, const gt4mi_field* diag,
                     const gt4mi_field* upper, const int64_t extent[3], int axis, int elem_size, int flags, void* workspace,
                     int64_t workspace_bytes, void* stream, int64_t* workspace_needed, int* path, int* launches) {
    return gt4mi::line_solve(out, rhs, nfields, lower, diag, upper, extent, axis, elem_size, flags, workspace, workspace_bytes,
                             static_cast<hipStream_t>(stream), workspace_needed, path, launches);
}

int gt4mi_line_scan(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* weight, const int64_t extent[3], int axis,
                    int elem_size, int op, int flags, void* stream, int* path, int* launches) {
    return gt4mi::line_scan(dst, src, nfields, weight, extent, axis, elem_size, op, flags, static_cast<hipStream_t>(stream), path, launches);
}

int gt4mi_line_find(const gt4mi_field* fields, int nfields, const gt4mi_field* coord, const int64_t extent[3], int axis, int elem_size,
                    int what, int direction, const double* level, double missing, double* result, int flags, void* stream, int* path,
                    int* launches) {
    return gt4mi::line_find(fields, nfields, coord, extent, axis, elem_size, what, direction, level, missing, result, flags,
                            static_cast<hipStream_t>(stream), path, launches);
}

int gt4mi_field_histogram(const gt4mi_field* fields, int nfields, const int64_t extent[3], int elem_size, int nbins, const double* edges,
                          const double* edges_host, int by, int64_t* result, int flags, void* stream, int* path, int* launches) {
    return gt4mi::field_histogram(fields, nfields, extent, elem_size, nbins, edges, edges_host, by, result, flags,
                                  static_cast<hipStream_t>(stream), path, launches);
}

int gt4mi_line_filter(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const double* response, const int64_t* response_extent,
                      const double* twiddles, double* result, const int64_t extent[3], int axis, int elem_size, int mode, int flags,
                      void* stream, int* path, int* launches) {
    return gt4mi::line_filter(dst, src, nfields, response, response_extent, twiddles, result, extent, axis, elem_size, mode, flags,
                              static_cast<hipStream_t>(stream), path, launches);
}

// ---- multi-GPU ----------------------------------------------------------------------------------
int gt4mi_comm_unique_id(void* id128) {
    if (id128 == nullptr) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "comm_unique_id: null buffer");
    if (!gt4mi::rccl().ok) return gt4mi::fail(GT4MI_ERR_UNSUPPORTED, "librccl could not be loaded");
    GT4MI_RCCL_CHECK(gt4mi::rccl().GetUniqueId(static_cast<gt4mi::RcclUniqueId*>(id128)));
    return GT4MI_OK;
}

int gt4mi_comm_create(const void* id128, int nranks, int rank, gt4mi_comm** comm) {
    if (id128 == nullptr || comm == nullptr || nranks < 1 || rank < 0 || rank >= nranks)
        return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "comm_create: invalid argument");
    if (!gt4mi::rccl().ok) return gt4mi::fail(GT4MI_ERR_UNSUPPORTED, "librccl could not be loaded");
    gt4mi::RcclUniqueId id;
    memcpy(&id, id128, sizeof id);
    gt4mi_comm* c = new gt4mi_comm;
    c->nranks = nranks;
    c->rank = rank;
    int r = gt4mi::rccl().CommInitRank(&c->comm, nranks, id, rank);
    if (r != 0) {
        delete c;
        return gt4mi::fail(GT4MI_ERR_HIP, "ncclCommInitRank failed: %s",
                           gt4mi::rccl().GetErrorString ? gt4mi::rccl().GetErrorString(r) : "rccl error");
    }
    *comm = c;
    return GT4MI_OK;
}

int gt4mi_comm_create_local(int nranks, int rank, gt4mi_comm** comm) {
    if (comm == nullptr || nranks < 1 || rank < 0 || rank >= nranks)
        return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "comm_create_local: invalid argument");
    gt4mi_comm* c = new gt4mi_comm;  // no RCCL communicator behind it: plans on it exchange through the direct transport only
    c->nranks = nranks;
    c->rank = rank;
    *comm = c;
    return GT4MI_OK;
}

int gt4mi_comm_info(gt4mi_comm* comm, int* nranks, int* rank, int* device) {
    if (comm == nullptr) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "comm_info: null communicator");
    if (comm->comm == nullptr) {  // gt4mi_comm_create_local: what the caller said, and the current device
        if (nranks) *nranks = comm->nranks;
        if (rank) *rank = comm->rank;
        if (device) GT4MI_HIP_CHECK(hipGetDevice(device));
        return GT4MI_OK;
    }
    gt4mi::RcclApi& api = gt4mi::rccl();
    // what RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice), not what the
    // caller passed to gt4mi_comm_create
    if (nranks) {
        if (!api.CommCount) return gt4mi::fail(GT4MI_ERR_UNSUPPORTED, "comm_info: ncclCommCount not available");
        GT4MI_RCCL_CHECK(api.CommCount(comm->comm, nranks));
    }
    if (rank) {
        if (!api.CommUserRank) return gt4mi::fail(GT4MI_ERR_UNSUPPORTED, "comm_info: ncclCommUserRank not available");
        GT4MI_RCCL_CHECK(api.CommUserRank(comm->comm, rank));
    }
    if (device) {
        if (!api.CommCuDevice) return gt4mi::fail(GT4MI_ERR_UNSUPPORTED, "comm_info: ncclCommCuDevice not available");
        GT4MI_RCCL_CHECK(api.CommCuDevice(comm->comm, device));
    }
    return GT4MI_OK;
}

int gt4mi_comm_destroy(gt4mi_comm* comm) {
    if (comm == nullptr) return GT4MI_OK;
    if (comm->comm) gt4mi::rccl().CommDestroy(comm->comm);
    delete comm;
    return GT4MI_OK;
}

int gt4mi_halo_plan_create(gt4mi_comm* comm, int elem_size, const gt4mi_halo_msg* sends, int nsends,
                           const gt4mi_halo_msg* recvs, int nrecvs, gt4mi_halo_plan** plan) {
    if (comm == nullptr || plan == nullptr || (nsends > 0 && sends == nullptr) || (nrecvs > 0 && recvs == nullptr))
        return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_create: null argument");
    if (elem_size != 4 && elem_size != 8)
        return gt4mi::fail(GT4MI_ERR_UNSUPPORTED, "halo_plan_create: element size %d", elem_size);
    gt4mi_halo_plan* p = new gt4mi_halo_plan;
    p->comm = comm;
    p->elem_size = elem_size;
    auto add = [&](const gt4mi_halo_msg& m, bool is_send) -> int {
        if (m.phase < 0 || m.phase > 1 || m.peer < 0 || m.peer >= comm->nranks)
            return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_create: bad phase/peer");
        gt4mi_halo_plan::Msg x;
        x.peer = m.peer;
        size_t n = 1;
        for (int a = 0; a < 3; ++a) {
            if (m.extent[a] < 0 || m.lo[a] < 0) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_create: bad box");
            x.lo[a] = m.lo[a];
            x.ext[a] = m.extent[a];
            n *= (size_t)m.extent[a];
        }
        x.bytes = n * (size_t)elem_size;
        x.buffer = nullptr;
        if (x.bytes) GT4MI_HIP_CHECK(hipMalloc(&x.buffer, x.bytes));
        (is_send ? p->sends : p->recvs)[m.phase].push_back(x);
        return GT4MI_OK;
    };
    int rc = GT4MI_OK;
    for (int i = 0; i < nsends && rc == GT4MI_OK; ++i) rc = add(sends[i], true);
    for (int i = 0; i < nrecvs && rc == GT4MI_OK; ++i) rc = add(recvs[i], false);
    if (rc == GT4MI_OK) {
        // Normal priority on purpose: measured on MI355X (1-rank self-loop rehearsal, 512x64x512 per
        // step) a highest-priority side stream made the step 3x SLOWER (0.267 ms vs 0.088 ms) and a
        // lowest-priority one 1.6x slower.
        if (hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess)
            rc = gt4mi::fail(GT4MI_ERR_HIP, "halo_plan_create: hipStreamCreate failed");
    }
    if (rc == GT4MI_OK && (hipEventCreateWithFlags(&p->ready, hipEventDisableTiming) != hipSuccess ||
                           hipEventCreateWithFlags(&p->done, hipEventDisableTiming) != hipSuccess))
        rc = gt4mi::fail(GT4MI_ERR_HIP, "halo_plan_create: hipEventCreate failed");
    if (rc == GT4MI_OK) {
        void* words = nullptr;
        if (hipMalloc(&words, 256) != hipSuccess || hipMemset(words, 0, 256) != hipSuccess)
            rc = gt4mi::fail(GT4MI_ERR_HIP, "halo_plan_create: hipMalloc failed");
        p->probe = static_cast<unsigned*>(words);
        p->edge_words = words ? reinterpret_cast<uint32_t*>(words) + 32 : nullptr;  // (the second half of the 256 bytes)
    }
    if (rc != GT4MI_OK) {
        gt4mi_halo_plan_destroy(p);
        return rc;
    }
    *plan = p;
    return GT4MI_OK;
}

int gt4mi_halo_plan_set_option(gt4mi_halo_plan* plan, int option, int value) {
    if (plan == nullptr) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_set_option: null plan");
    switch (option) {
        case GT4MI_PLAN_SCHEDULE:
            if (value < -1 || value > GT4MI_SCHEDULE_INLINE) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_set_option: schedule %d", value);
            plan->schedule = value;
            return GT4MI_OK;
        case GT4MI_PLAN_EDGE_COLUMNS:
            if (value < -1 || value > 4096) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_set_option: %d edge columns", value);
            plan->edge_columns = value;
            return GT4MI_OK;
        case GT4MI_PLAN_DEFER_JOIN:
            if (value != 0 && value != 1) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_set_option: defer_join %d", value);
            plan->defer_join = value;
            return GT4MI_OK;
        case GT4MI_PLAN_INTERIOR_WG_PER_CU:
            if (value < -1 || value > 16) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_set_option: %d workgroups per CU", value);
            plan->interior_wg_per_cu = value;
            return GT4MI_OK;
        case GT4MI_PLAN_TRANSPORT:
            if (value != GT4MI_TRANSPORT_RCCL && value != GT4MI_TRANSPORT_DIRECT)
                return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_set_option: transport %d", value);
            if (value == GT4MI_TRANSPORT_DIRECT) {
                if (!plan->direct.prepared)
                    return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_set_option: prepare and connect the direct transport first "
                                                                   "(gt4mi_halo_plan_direct_prepare / _connect)");
                for (int ph = 0; ph < 2; ++ph) {
                    for (size_t m = 0; m < plan->sends[ph].size(); ++m)
                        if (!plan->direct.send_to[ph][m] || !plan->direct.signal_arrived[ph][m])
                            return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_set_option: send %d of phase %d is not connected", (int)m, ph);
                    for (size_t m = 0; m < plan->recvs[ph].size(); ++m)
                        if (!plan->direct.signal_consumed[ph][m])
                            return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_set_option: receive %d of phase %d is not connected", (int)m, ph);
                }
            }
            plan->transport = value;
            return GT4MI_OK;
        case GT4MI_PLAN_DIRECT_TIMEOUT_MS:
            if (value < 0) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_set_option: a timeout of %d ms", value);
            plan->direct.timeout_ms = value;
            return GT4MI_OK;
        case GT4MI_PLAN_DIRECT_FENCED:
            if (value != 0 && value != 1) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_set_option: direct_fenced %d", value);
            plan->direct.fenced = value;
            return GT4MI_OK;
    }
    return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_set_option: unknown option %d", option);
}

int gt4mi_halo_plan_concurrent(gt4mi_halo_plan* plan) {
    if (plan == nullptr) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_concurrent: null plan");
    return plan->probed ? (plan->concurrent ? 1 : 0) : 2;
}

int gt4mi_halo_plan_direct_prepare(gt4mi_halo_plan* plan, gt4mi_direct_info* info) {
    if (plan == nullptr) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_direct_prepare: null plan");
    return gt4mi::direct_prepare(plan, info);
}

int gt4mi_halo_plan_direct_layout(gt4mi_halo_plan* plan, int phase, int is_send, int index, int64_t* pool_offset, int* flag_index) {
    if (plan == nullptr || !plan->direct.prepared) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_direct_layout: not prepared");
    if (phase < 0 || phase > 1) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_direct_layout: phase %d", phase);
    const size_t n = is_send ? plan->sends[phase].size() : plan->recvs[phase].size();
    if (index < 0 || (size_t)index >= n) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_direct_layout: message %d of %d", index, (int)n);
    if (pool_offset) *pool_offset = is_send ? -1 : (int64_t)plan->direct.recv_offset[phase][index];
    if (flag_index) *flag_index = gt4mi::direct_index(plan, is_send != 0, phase, index);
    return GT4MI_OK;
}

int gt4mi_halo_plan_direct_connect(gt4mi_halo_plan* plan, int phase, int is_send, int index, const gt4mi_direct_info* peer,
                                   int64_t peer_pool_offset, int peer_flag_index) {
    if (plan == nullptr) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_direct_connect: null plan");
    return gt4mi::direct_connect(plan, phase, is_send, index, peer, peer_pool_offset, peer_flag_index);
}

int gt4mi_halo_plan_direct_status(gt4mi_halo_plan* plan, int* timed_out, unsigned* exchanges) {
    if (plan == nullptr || !plan->direct.prepared) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_plan_direct_status: not prepared");
    GT4MI_HIP_CHECK(hipDeviceSynchronize());  // every exchange started so far has either completed or given up
    const uint32_t word = __atomic_load_n(plan->direct.error, __ATOMIC_RELAXED);  // (host memory the device writes)
    if (timed_out) *timed_out = (int)word;
    if (exchanges) *exchanges = plan->direct.step;
    return GT4MI_OK;
}

int gt4mi_halo_plan_destroy(gt4mi_halo_plan* plan) {
    if (plan == nullptr) return GT4MI_OK;
    gt4mi::direct_release(plan);  // (the receive buffers of a prepared plan live in its pool)
    for (int ph = 0; ph < 2; ++ph) {
        for (auto& m : plan->sends[ph]) if (m.buffer) (void)hipFree(m.buffer);
        for (auto& m : plan->recvs[ph]) if (m.buffer) (void)hipFree(m.buffer);
    }
    if (plan->probe) (void)hipFree(plan->probe);
    if (plan->ready) (void)hipEventDestroy(plan->ready);
    if (plan->done) (void)hipEventDestroy(plan->done);
    if (plan->stream) (void)hipStreamDestroy(plan->stream);
    delete plan;
    return GT4MI_OK;
}

int gt4mi_halo_exchange(gt4mi_halo_plan* plan, const gt4mi_field* field, void* stream) {
    if (plan == nullptr || field == nullptr) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_exchange: null argument");
    return gt4mi::halo_exchange_on(plan, field, static_cast<hipStream_t>(stream));
}

int gt4mi_halo_exchange_fork(gt4mi_halo_plan* plan, void* main_stream) {
    if (plan == nullptr) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_exchange_fork: null plan");
    // first use with this stream: make sure the side stream does not share its hardware queue (one-off,
    // synchronising probe) -- otherwise the "overlapped" exchange simply queues behind the interior kernel
    if (int rc = gt4mi::ensure_concurrent_stream(plan, static_cast<hipStream_t>(main_stream))) return rc;
    if (int rc = gt4mi::record_ready(plan, static_cast<hipStream_t>(main_stream))) return rc;
    plan->forked = true;
    return GT4MI_OK;
}

int gt4mi_halo_exchange_begin(gt4mi_halo_plan* plan, const gt4mi_field* field, void* main_stream) {
    if (plan == nullptr || field == nullptr) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_exchange_begin: null argument");
    if (!plan->forked)
        if (int rc = gt4mi::ensure_concurrent_stream(plan, static_cast<hipStream_t>(main_stream))) return rc;
    if (!plan->forked)
        if (int rc = gt4mi::record_ready(plan, static_cast<hipStream_t>(main_stream))) return rc;
    plan->forked = false;
    if (int rc = gt4mi::side_waits_ready(plan)) return rc;
    if (int rc = gt4mi::halo_exchange_on(plan, field, plan->stream)) return rc;
    if (int rc = gt4mi::mark_done(plan)) return rc;
    plan->primed = true;
    return GT4MI_OK;
}

int gt4mi_halo_exchange_end(gt4mi_halo_plan* plan, void* main_stream) {
    if (plan == nullptr) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_exchange_end: null plan");
    return gt4mi::join_side_now(plan, static_cast<hipStream_t>(main_stream));
}

int gt4mi_dist_lap5_f64(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* inp,
                        const gt4mi_field* out, int variant, int sides, void* main_stream) {
    return gt4mi::dist_lap5<double, double>(plan, domain, inp, out, variant, sides, main_stream);
}

int gt4mi_dist_lap5_query(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* out, int sides,
                          int* edge_units) {
    if (plan == nullptr || inp == nullptr || out == nullptr || domain == nullptr || edge_units == nullptr)
        return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "dist_lap5_query: null argument");
    bool ok = false;
    const int rc = plan->elem_size == 8 ? gt4mi::lap5_edge_units_qualify<double>(plan, domain, inp, out, sides, &ok)
                                        : gt4mi::lap5_edge_units_qualify<float>(plan, domain, inp, out, sides, &ok);
    *edge_units = ok ? 1 : 0;
    return rc;
}

int gt4mi_dist_lap5_f32(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* inp,
                        const gt4mi_field* out, int variant, int flags, int sides, void* main_stream) {
    if (flags & GT4MI_LAP_LITERAL_F32) return gt4mi::dist_lap5<float, float>(plan, domain, inp, out, variant, sides, main_stream);
    return gt4mi::dist_lap5<float, double>(plan, domain, inp, out, variant, sides, main_stream);
}

int gt4mi_dist_lap5_f64_wide(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* inp,
                             const gt4mi_field* out, int variant, int sides, int halo, int phase, void* main_stream) {
    return gt4mi::dist_lap5_wide(plan, domain, inp, out, variant, sides, halo, phase, main_stream);
}

int gt4mi_dist_lap5_f64_skewed(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* field_a,
                               const gt4mi_field* field_b, int variant, int sides, int halo, void* main_stream) {
    return gt4mi::dist_lap5_skewed(plan, domain, field_a, field_b, variant, sides, halo, main_stream);
}

int gt4mi_dist_lap5_f64_pipelined(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* inp,
                                  const gt4mi_field* out, int variant, int sides, void* main_stream) {
    return gt4mi_dist_lap5_f64_wide(plan, domain, inp, out, variant, sides, 1, 0, main_stream);
}

int gt4mi_dist_hdiff_f64(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* in_field,
                         const gt4mi_field* out_field, const gt4mi_field* coeff, double coeff_scalar, int flags, int sides,
                         void* main_stream) {
    return gt4mi::dist_hdiff<double>(plan, domain, in_field, out_field, coeff, coeff_scalar, flags, sides, main_stream);
}

int gt4mi_dist_hdiff_f32(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* in_field,
                         const gt4mi_field* out_field, const gt4mi_field* coeff, double coeff_scalar, int flags, int sides,
                         void* main_stream) {
    return gt4mi::dist_hdiff<float>(plan, domain, in_field, out_field, coeff, coeff_scalar, flags, sides, main_stream);
}

int gt4mi_stream_copy(const void* src, void* dst, size_t nbytes, void* stream) {
    if (src == nullptr || dst == nullptr) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "stream_copy: null pointer");
    if (nbytes % 16 != 0 || (reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 16 != 0)
        return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "stream_copy: pointers and size must be multiples of 16 bytes");
    const size_t nvec = nbytes / 16;
    if (nvec == 0) return GT4MI_OK;
    // best of the variants in `microbench copy` (profiles/r1_microbench_*.log): one 16-byte vector per
    // thread, no grid-stride loop, non-temporal stores -- 6.23 TB/s on MI355X
    constexpr int UNROLL = 1;
    size_t blocks = (nvec + 255) / 256;
    if (blocks > 0x7fffffffull) blocks = 0x7fffffffull;
    hipLaunchKernelGGL((gt4mi::stream_copy_kernel<UNROLL, true>), dim3((unsigned)blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<const gt4mi::u32x4*>(src),
                       static_cast<gt4mi::u32x4*>(dst), nvec);
    GT4MI_HIP_CHECK(hipGetLastError());
    return GT4MI_OK;
}

int gt4mi_memory_write_probe(void* a, void* b, size_t bytes, int iterations, void* stream, double* gbs) {
    return gt4mi::memory_write_probe(a, b, bytes, iterations, static_cast<hipStream_t>(stream), gbs);
}

// ---- run-time compiled stencils (generic executor) -------------------------------------------------

int gt4mi_rtc_compile(const char* source, const char* name, const char* const* options, int n_options,
                      void** code, size_t* code_size, char* log, size_t log_size) {
    return gt4mi::rtc_compile(source, name, options, n_options, code, code_size, log, log_size);
}

int gt4mi_rtc_free(void* code) {
    free(code);
    return GT4MI_OK;
}

int gt4mi_module_load(const void* code, gt4mi_module** module) {
    if (code == nullptr || module == nullptr) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "module_load: null argument");
    auto* m = new gt4mi_module();
    hipError_t e = hipModuleLoadData(&m->module, code);
    if (e != hipSuccess) {
        delete m;
        return gt4mi::fail(GT4MI_ERR_HIP, "hipModuleLoadData failed: %s", hipGetErrorString(e));
    }
    *module = m;
    return GT4MI_OK;
}

int gt4mi_module_unload(gt4mi_module* module) {
    if (module == nullptr) return GT4MI_OK;
    hipError_t e = module->module ? hipModuleUnload(module->module) : hipSuccess;
    delete module;
    if (e != hipSuccess) return gt4mi::fail(GT4MI_ERR_HIP, "hipModuleUnload failed: %s", hipGetErrorString(e));
    return GT4MI_OK;
}

int gt4mi_module_function(gt4mi_module* module, const char* name, void** function) {
    if (module == nullptr || name == nullptr || function == nullptr)
        return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "module_function: null argument");
    hipFunction_t fn = nullptr;
    hipError_t e = hipModuleGetFunction(&fn, module->module, name);
    if (e != hipSuccess)
        return gt4mi::fail(GT4MI_ERR_HIP, "hipModuleGetFunction(%s) failed: %s", name, hipGetErrorString(e));
    *function = fn;
    return GT4MI_OK;
}

int gt4mi_function_info(void* function, int* registers, int* scratch_bytes, int* lds_bytes) {
    if (function == nullptr) return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "function_info: null function");
    hipFunction_t fn = static_cast<hipFunction_t>(function);
    int v = 0;
    if (registers) {
        GT4MI_HIP_CHECK(hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_NUM_REGS, fn));
        *registers = v;
    }
    if (scratch_bytes) {
        GT4MI_HIP_CHECK(hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, fn));
        *scratch_bytes = v;
    }
    if (lds_bytes) {
        GT4MI_HIP_CHECK(hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, fn));
        *lds_bytes = v;
    }
    return GT4MI_OK;
}

int gt4mi_launch(void* function, const uint32_t grid[3], const uint32_t block[3], const void* args,
                 size_t args_size, void* stream, gt4mi_exec_info* info) {
    Timer timer(info, stream);
    if (function == nullptr || grid == nullptr || block == nullptr || (args == nullptr && args_size != 0))
        return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "launch: null argument");
    if (grid[0] == 0 || grid[1] == 0 || grid[2] == 0) return GT4MI_OK;  // empty iteration space
    if ((size_t)block[0] * block[1] * block[2] > 1024 || block[0] * block[1] * block[2] == 0)
        return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "launch: workgroup of %u x %u x %u threads", block[0],
                           block[1], block[2]);
    if (grid[1] > 65535u || grid[2] > 65535u)
        return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "launch: grid %u x %u x %u exceeds 65535 in y or z", grid[0],
                           grid[1], grid[2]);
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, const_cast<void*>(args), HIP_LAUNCH_PARAM_BUFFER_SIZE,
                     &args_size, HIP_LAUNCH_PARAM_END};
    GT4MI_HIP_CHECK(hipModuleLaunchKernel(static_cast<hipFunction_t>(function), grid[0], grid[1], grid[2], block[0],
                                          block[1], block[2], 0, static_cast<hipStream_t>(stream), nullptr, extra));
    return GT4MI_OK;
}

int gt4mi_launch_batch(int n, void* const* functions, const uint32_t* grids, const uint32_t* blocks,
                       const void* const* args, size_t args_size, void* stream, gt4mi_exec_info* info) {
    Timer timer(info, stream);
    if (n < 0 || (n > 0 && (functions == nullptr || grids == nullptr || blocks == nullptr || args == nullptr)))
        return gt4mi::fail(GT4MI_ERR_INVALID_ARGUMENT, "launch_batch: null argument");
    for (int l = 0; l < n; ++l) {
        const int rc = gt4mi_launch(functions[l], grids + 3 * l, blocks + 3 * l, args[l], args_size, stream, nullptr);
        if (rc != GT4MI_OK) return rc;
    }
    return GT4MI_OK;
}

}  // extern "C"
