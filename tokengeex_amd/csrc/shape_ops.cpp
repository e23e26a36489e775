// The C ABI's shapes over a resident corpus (include/tgx_shapes.h: tgx_corpus_shape_hits_device,
// tgx_corpus_shape_cover_device, tgx_shapes_last_times): the shapes' and the arguments' checks, the table's build and
// upload, the cover's scratch for the ends and the stages' times around the launchers of shape.hip.  The calls run on the
// caller's stream under a StreamGuard, as the automaton of dfa_ops.cpp does, and share device_internal.h with it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/tgx_shapes.h"
#include "api_internal.h"
#include "device_internal.h"
#include "shape.h"

using namespace tgx::host;
using namespace tgx::dev;

static_assert(TGX_SHAPES_MAX_PATTERNS == tgx::kShapesMaxPatterns && TGX_SHAPE_MAX_LEN == tgx::kShapeMaxLen && TGX_SHAPES_MAX_BITS == tgx::kShapesMaxBits &&
                  sizeof(tgx_shapes) == 4 + 8 * 4 + 128 * 32 + 2 * 8 * 32,
              "include/tgx_shapes.h and shape.h name the same shapes");

namespace {

const char* const kShapeStageNames[tgx::kShapeStages] = {"shape_ends_kernel", "shape_cover_kernel"};
thread_local float g_shape_ms[tgx::kShapeStages] = {0, 0};

// What the two calls share.  cover: the second kernel runs too, on the ends of the first in pooled scratch; out_rows is
// count or covered and out_bytes ends or mask.
tgx_status shape_call(const char* who, tgx_corpus* c, const tgx_shapes* shp, bool cover, const char* rows_name, const char* bytes_name, int64_t* d_out_rows,
                      uint8_t* d_out_bytes, void* stream) {
    tgx_status st = require_device();
    if (st != TGX_OK) return st;
    if (!c || !shp) return fail(TGX_ERR_INVALID, "%s: %s is NULL", who, c ? "shapes" : "corpus");
    if (const char* why = tgx::shape_check(shp->n_patterns, shp->len, shp->cls)) return fail(TGX_ERR_INVALID, "%s: %s", who, why);
    const uint32_t nw = tgx::shape_nw(tgx::shape_total(shp->n_patterns, shp->len));
    std::vector<uint64_t> table(nw == 1 ? tgx::kShapeTableWords<1> : tgx::kShapeTableWords<2>);
    if (nw == 1)
        tgx::shape_build_table<1>(shp->n_patterns, shp->len, shp->cls, shp->not_before, shp->not_after, table.data());
    else
        tgx::shape_build_table<2>(shp->n_patterns, shp->len, shp->cls, shp->not_before, shp->not_after, table.data());
    std::lock_guard<std::mutex> lkc(c->mu);
    if (!d_out_rows && !d_out_bytes) return fail(TGX_ERR_INVALID, "%s: %s and %s are both NULL", who, rows_name, bytes_name);
    const tgx::DedupRows rows{c->d_text, c->d_offs.get(), c->n_samples, c->n_bytes, 1};
    const uint64_t S = rows.n_rows;
    if (S >= 0xFFFFFFFFull) return fail(TGX_ERR_UNSUPPORTED, "%s: more than 2^32-1 rows", who);
    const int n_stages = cover ? 2 : 1;
    if (S == 0) {
        std::fill(g_shape_ms, g_shape_ms + n_stages, 0.0f);
        return TGX_OK;
    }
    const int device = c->device;
    DeviceScope scope;
    HIP_TRY(hipSetDevice(device));
    if ((st = check_device_ptr(who, rows_name, d_out_rows, device, "corpus")) != TGX_OK) return st;
    if ((st = check_device_ptr(who, bytes_name, d_out_bytes, device, "corpus")) != TGX_OK) return st;
    hipStream_t hs = stream_or_default(stream, device);
    float ms[tgx::kShapeStages] = {0, 0};
    StageTimer<tgx::kShapeStages> timer(hs, ms);  // (before the guard: its events outlive the stream's work)
    StreamGuard guard(device, hs);
    if (rows.n_elems) {
        uint64_t* d_table = nullptr;
        uint8_t* d_ends = nullptr;  // the cover's: every byte is written by the first kernel, whatever the pool held
        if (guard.alloc(table.size() * 8, &d_table) != hipSuccess || (cover && guard.alloc((size_t)rows.n_elems, &d_ends) != hipSuccess)) {
            (void)hipGetLastError();
            return fail(TGX_ERR_DEVICE, "out of device memory (shapes)");
        }
        HIP_TRY(guard.upload(d_table, std::move(table)));  // (the guard keeps the host words until the stream's end)
        timer.begin(0);
        if (tgx::launch_shape_ends(rows, nw, d_table, cover ? nullptr : d_out_rows, cover ? d_ends : d_out_bytes, hs) != hipSuccess)
            return fail(TGX_ERR_DEVICE, "shape_ends_kernel launch failed");
        timer.end(0);
        if (cover) {
            timer.begin(1);
            if (tgx::launch_shape_cover(rows, shp->n_patterns, shp->len, d_ends, d_out_rows, d_out_bytes, hs) != hipSuccess)
                return fail(TGX_ERR_DEVICE, "shape_cover_kernel launch failed");
            timer.end(1);
        }
    } else if ((cover ? tgx::launch_shape_cover(rows, shp->n_patterns, shp->len, nullptr, d_out_rows, nullptr, hs)
                      : tgx::launch_shape_ends(rows, nw, nullptr, d_out_rows, nullptr, hs)) != hipSuccess) {  // only empty rows: the sums' zeros
        return fail(TGX_ERR_DEVICE, "%s: the pre-set failed", who);
    }
    HIP_TRY(hipStreamSynchronize(hs));
    guard.done();
    timer.read();
    std::copy(ms, ms + n_stages, g_shape_ms);
    return TGX_OK;
}

}  // namespace

int tgx_shapes_last_times(const char** names, float* ms, int cap) { return stage_times(kShapeStageNames, g_shape_ms, tgx::kShapeStages, names, ms, cap); }

tgx_status tgx_corpus_shape_hits_device(tgx_corpus* c, const tgx_shapes* shapes, int64_t* d_count, uint8_t* d_ends, void* stream) {
    return shape_call("tgx_corpus_shape_hits_device", c, shapes, false, "count", "ends", d_count, d_ends, stream);
}

tgx_status tgx_corpus_shape_cover_device(tgx_corpus* c, const tgx_shapes* shapes, int64_t* d_covered, uint8_t* d_mask, void* stream) {
    return shape_call("tgx_corpus_shape_cover_device", c, shapes, true, "covered", "mask", d_covered, d_mask, stream);
}
