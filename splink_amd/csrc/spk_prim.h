// Device-wide primitives (rocprim) behind the project's error codes.  Included only by the translation units
// that sort or scan, so the others do not compile rocprim.
//
// Every rocprim call comes in two: with a null scratch pointer it reports the scratch size, with the scratch it
// runs.  Each wrapper takes the stream and a scratch buffer that grows as needed and can be handed from call
// to call; n == 0 does nothing.  Inputs are plain (non-const) pointers: rocprim instantiates its kernels per
// iterator type, and one type per primitive keeps one set of them in the library.
#pragma once

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_scan.hpp>

#include "spk_internal.h"

namespace spk {

// call(scratch, bytes) -> hipError_t: once for the size, once to run.
template <typename Call>
inline int prim_two_calls(const char *what, DevBuf<uint8_t> &tmp, Call call) {
    size_t bytes = 0;
    hipError_t e = call(static_cast<void *>(nullptr), bytes);
    if (e == hipSuccess) {
        SPK_TRY(tmp.alloc(bytes + 1));
        e = call(static_cast<void *>(tmp.p), bytes);
    }
    if (e != hipSuccess) {
        set_error(std::string(what) + ": " + hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SPK_E_OOM : SPK_E_HIP;
    }
    return SPK_OK;
}

// Stable sort of (key, value) pairs by the low `bits` bits of the key (the higher ones are not compared).
template <typename V>
inline int sort_pairs_u64(hipStream_t stream, DevBuf<uint8_t> &tmp, uint64_t *keys_in, uint64_t *keys_out, V *vals_in,
                          V *vals_out, int64_t n, int bits = 64) {
    if (n <= 0) return SPK_OK;
    return prim_two_calls("rocprim::radix_sort_pairs", tmp, [&](void *scratch, size_t &bytes) {
        return rocprim::radix_sort_pairs(scratch, bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0,
                                         (unsigned int)bits, stream);
    });
}

// Sort of keys by their low `bits` bits.
inline int sort_keys_u64(hipStream_t stream, DevBuf<uint8_t> &tmp, uint64_t *keys_in, uint64_t *keys_out, int64_t n,
                         int bits = 64) {
    if (n <= 0) return SPK_OK;
    return prim_two_calls("rocprim::radix_sort_keys", tmp, [&](void *scratch, size_t &bytes) {
        return rocprim::radix_sort_keys(scratch, bytes, keys_in, keys_out, (size_t)n, 0, (unsigned int)bits, stream);
    });
}

// out[i] = in[0] + .. + in[i - 1]
template <typename T>
inline int exclusive_scan(hipStream_t stream, DevBuf<uint8_t> &tmp, T *in, T *out, int64_t n) {
    if (n <= 0) return SPK_OK;
    return prim_two_calls("rocprim::exclusive_scan", tmp, [&](void *scratch, size_t &bytes) {
        return rocprim::exclusive_scan(scratch, bytes, in, out, (T)0, (size_t)n, rocprim::plus<T>(), stream);
    });
}

// out[i] = in[0] + .. + in[i]
template <typename T>
inline int inclusive_scan(hipStream_t stream, DevBuf<uint8_t> &tmp, T *in, T *out, int64_t n) {
    if (n <= 0) return SPK_OK;
    return prim_two_calls("rocprim::inclusive_scan", tmp, [&](void *scratch, size_t &bytes) {
        return rocprim::inclusive_scan(scratch, bytes, in, out, (size_t)n, rocprim::plus<T>(), stream);
    });
}

// out[i] = in[0] op .. op in[i] for an associative op over a value type of the caller's
template <typename T, typename Op>
inline int inclusive_scan_op(hipStream_t stream, DevBuf<uint8_t> &tmp, T *in, T *out, int64_t n, Op op) {
    if (n <= 0) return SPK_OK;
    return prim_two_calls("rocprim::inclusive_scan", tmp, [&](void *scratch, size_t &bytes) {
        return rocprim::inclusive_scan(scratch, bytes, in, out, (size_t)n, op, stream);
    });
}

// Counts, their exclusive prefix sums and their total.  Four things have this shape: the head flags of a
// sorted view (prefix: the block of every position, total: the number of blocks), a rule's candidates per block
// (prefix: the first ordinal of every block), the pairs a compaction pass keeps per chunk (prefix: where the
// emit pass writes every chunk's pairs), and the pairs a selection keeps per chunk (spk_select.hip, the same).
struct CountScan {
    DevBuf<int64_t> count, off;  // [n + 1]: count[n] is a zero that is scanned with the rest, so off[n] is the total
    int64_t n = 0, total = 0;
    int alloc(spk_ctx *ctx, int64_t n_counts) {
        n = n_counts;
        SPK_TRY(count.alloc((size_t)n + 1));
        SPK_TRY(off.alloc((size_t)n + 1));
        SPK_HIP(hipMemsetAsync(count.p + n, 0, sizeof(int64_t), ctx->stream));
        return SPK_OK;
    }
};

// Enqueued behind the kernel that writes S.count[0 .. n): the scan, then the read-back of the total.  Returns with
// the stream synchronised; the open interval of `T` (optional) ends between the scan and the read-back and is added.
inline int scan_total(spk_ctx *ctx, CountScan &S, DevBuf<uint8_t> &tmp, StageTimer *T = nullptr) {
    SPK_TRY(exclusive_scan(ctx->stream, tmp, S.count.p, S.off.p, S.n + 1));
    if (T) SPK_TRY(T->stop());
    SPK_HIP(hipMemcpyAsync(&S.total, S.off.p + S.n, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    SPK_HIP(hipStreamSynchronize(ctx->stream));
    return T ? T->add() : SPK_OK;
}

// *out = in[0] + .. + in[n - 1], summed as Out
template <typename In, typename Out>
inline int reduce_sum(hipStream_t stream, DevBuf<uint8_t> &tmp, In *in, Out *out, int64_t n) {
    if (n <= 0) return SPK_OK;
    return prim_two_calls("rocprim::reduce", tmp, [&](void *scratch, size_t &bytes) {
        return rocprim::reduce(scratch, bytes, in, out, (size_t)n, rocprim::plus<Out>(), stream);
    });
}

}  // namespace spk
