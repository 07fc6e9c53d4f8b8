// items.hpp -- the ragged passes of an item set (include/lcfir.h,
// lcfir_items_*): many files of different lengths laid out as rows of one
// arena, filtered group by group with the ordinary multi-channel launches.
//
// A group's launch runs with x_hi = end = N_g, the group's longest row, so a
// shorter row's outputs [n_f, N_g) hold the filter's ringing tail.  The fused
// peak would take them in; the per-file post-passes (ProcessFile.cp:91-101)
// and the codec either side (ProcessFile.cp:40-41, :115-117) therefore get
// forms that stop at each file's own n_f, and so do the two passes that move
// rows between the arenas and tensors of the caller's.  All walk a flat tile table
// built on the host when the item set is created:
//
//   row passes   (peak, normalize, gather, scatter):
//                                   tile -> (arena offset, floats, file),
//                                   kItemRowTile floats of one row;
//   codec passes (decode, encode):  tile -> (first interleaved sample, samples,
//                                   file), kItemPcmTile samples of one file.
//
// Tiles have one size whatever the file, so one launch balances a 60-minute
// file against a thousand 0.1 s ones, and the launch count does not grow with
// the rows.  Every row starts 16-byte aligned and every row tile starts a
// multiple of four floats into its row, so the row passes move float4s;
// each thread has kItemLoads of them in flight (peak_scale.hpp's reasoning).
// The sample rules themselves are codec.hpp's and peak_scale.hpp's
// (decode_one, encode_one_dither, split_sample, rescale_rule, scale_one,
// wave_max), so every value is the per-file call's bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec.hpp"
#include "peak_scale.hpp"

namespace lcfir {

constexpr int kItemThreads = 256;
constexpr int kItemLoads = 4;                                  // 16-byte loads in flight per thread
constexpr int kItemRowTile = kItemThreads * kItemLoads * 4;    // floats of a row per tile
constexpr int kItemPcmLoads = 8;                               // samples in flight per thread
constexpr int kItemPcmTile = kItemThreads * kItemPcmLoads;     // interleaved samples per tile

struct ItemTile {
    int64_t first; // row passes: offset of the tile in the arena, floats (a multiple of 4);
                   // codec passes: the tile's first interleaved sample of its file
    int32_t count; // floats / samples in the tile (<= the tile size)
    int32_t file;
};

// A file's block of rows, as the codec passes need it.
struct ItemFile {
    int64_t off;    // arena offset of channel 0, floats
    int64_t stride; // floats between channels
    int32_t nch;
    int32_t pad_;
};

// Per call: where a file's interleaved payload sits and how it is encoded.
struct ItemPcm {
    int64_t byte_off;
    PcmFormat f;
};

// max |y| of every file over its channels' [0, n_f): one wave reduction per
// tile, then one atomicMax on the float's bit pattern per wave and file.
// NaN is skipped (fmaxf), Inf taken -- peak_kernel's rule.
__global__ __launch_bounds__(kItemThreads) void items_peak_kernel(const float *__restrict__ y,
                                                                  const ItemTile *__restrict__ tiles,
                                                                  int64_t ntiles,
                                                                  unsigned *__restrict__ peak) {
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const ItemTile tl = tiles[t];
        const float *__restrict__ p = y + tl.first;
        const float4 *__restrict__ p4 = reinterpret_cast<const float4 *>(p);
        const int n4 = tl.count >> 2;
        float4 v[kItemLoads];
#pragma unroll
        for (int u = 0; u < kItemLoads; ++u) {
            const int i = (int)threadIdx.x + u * kItemThreads;
            v[u] = i < n4 ? p4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        float m = 0.0f;
        const int r = n4 * 4 + (int)threadIdx.x; // the row's last 1-3 floats
        if (r < tl.count) m = fabsf(p[r]);
#pragma unroll
        for (int u = 0; u < kItemLoads; ++u)
            m = fmaxf(m, fmaxf(fmaxf(fabsf(v[u].x), fabsf(v[u].y)), fmaxf(fabsf(v[u].z), fabsf(v[u].w))));
        m = wave_max(m);
        if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(peak + tl.file, __float_as_uint(m));
    }
}

// normalize_kernel's decision and rescale, file by file: rows [0, n_f) of
// file f become scale_one(y, 1 / peak[f]) iff (peak[f] > 1 or force) and
// peak[f] > 0.  A tile of a file that stays as it is costs one table entry
// and one peak load.
__global__ __launch_bounds__(kItemThreads) void items_normalize_kernel(float *__restrict__ y,
                                                                       const ItemTile *__restrict__ tiles,
                                                                       int64_t ntiles,
                                                                       const unsigned *__restrict__ peak,
                                                                       int force) {
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const ItemTile tl = tiles[t];
        const Rescale rs = rescale_rule(__uint_as_float(peak[tl.file]), force);
        if (!rs.on) continue;
        const double gain = rs.gain;
        float *__restrict__ p = y + tl.first;
        float4 *__restrict__ p4 = reinterpret_cast<float4 *>(p);
        const int n4 = tl.count >> 2;
        float4 v[kItemLoads];
#pragma unroll
        for (int u = 0; u < kItemLoads; ++u) {
            const int i = (int)threadIdx.x + u * kItemThreads;
            if (i < n4) v[u] = p4[i];
        }
#pragma unroll
        for (int u = 0; u < kItemLoads; ++u) {
            const int i = (int)threadIdx.x + u * kItemThreads;
            if (i < n4) {
                v[u].x = scale_one(v[u].x, gain);
                v[u].y = scale_one(v[u].y, gain);
                v[u].z = scale_one(v[u].z, gain);
                v[u].w = scale_one(v[u].w, gain);
                p4[i] = v[u];
            }
        }
        const int r = n4 * 4 + (int)threadIdx.x;
        if (r < tl.count) p[r] = scale_one(p[r], gain);
    }
}

// Per call of the tensor passes: where file f's rows sit in the caller's own
// memory (channel c at ptr + c * stride; only 4-byte alignment is asked of it).
struct ItemSpan {
    float *ptr;
    int64_t stride;
};

constexpr int kItemDwordLoads = 16; // dword loads in flight per thread where the caller's side is unaligned

// A row tile's place in the caller's memory: the tile's channel and position
// in its row follow from the two tables (rows of a file are `stride` apart in
// the arena, so the quotient is the channel), wave-uniform per tile.
__device__ __forceinline__ float *item_span_ptr(const ItemTile &tl, const ItemFile &fl, const ItemSpan &sp) {
    const int64_t rel = tl.first - fl.off;
    const int64_t c = rel / fl.stride;
    const int64_t t0 = rel - c * fl.stride;
    return sp.ptr + c * sp.stride + t0;
}

// The way in for rows that already sit in device memory of the caller's:
// floats [t0, t0 + count) of row c of span[f] go to the tile's place in the
// input arena.  Values are only moved (as 32-bit words, so every bit pattern
// survives), and only [0, n_f) of a row is written: the padding stays zero.
// The arena side is 16-byte aligned; where the source is too the tile moves
// float4s like the other row passes, else dwords, sixteen in flight.
__global__ __launch_bounds__(kItemThreads, 8) void items_gather_kernel(float *__restrict__ x,
                                                                    const ItemTile *__restrict__ tiles,
                                                                    int64_t ntiles,
                                                                    const ItemFile *__restrict__ files,
                                                                    const ItemSpan *__restrict__ span) {
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const ItemTile tl = tiles[t];
        const uint32_t *__restrict__ src =
            reinterpret_cast<const uint32_t *>(item_span_ptr(tl, files[tl.file], span[tl.file]));
        uint32_t *__restrict__ dst = reinterpret_cast<uint32_t *>(x + tl.first);
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const uint4 *__restrict__ s4 = reinterpret_cast<const uint4 *>(src);
            uint4 *__restrict__ d4 = reinterpret_cast<uint4 *>(dst);
            const int n4 = tl.count >> 2;
            uint4 v[kItemLoads];
#pragma unroll
            for (int u = 0; u < kItemLoads; ++u) {
                const int i = (int)threadIdx.x + u * kItemThreads;
                v[u] = i < n4 ? s4[i] : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int u = 0; u < kItemLoads; ++u) {
                const int i = (int)threadIdx.x + u * kItemThreads;
                if (i < n4) d4[i] = v[u];
            }
            const int r = n4 * 4 + (int)threadIdx.x; // the row's last 1-3 floats
            if (r < tl.count) dst[r] = src[r];
        } else {
            uint32_t v[kItemDwordLoads];
#pragma unroll
            for (int u = 0; u < kItemDwordLoads; ++u) {
                const int i = (int)threadIdx.x + u * kItemThreads;
                v[u] = i < tl.count ? src[i] : 0u;
            }
#pragma unroll
            for (int u = 0; u < kItemDwordLoads; ++u) {
                const int i = (int)threadIdx.x + u * kItemThreads;
                if (i < tl.count) dst[i] = v[u];
            }
        }
    }
}

// The way out, with items_normalize_kernel's rescale on the way: file f's rows
// [0, n_f) of the output arena go to span[f] as scale_one(y, 1 / peak[f]) iff
// (peak[f] > 1 or force) and peak[f] > 0, else as they are (peak == nullptr: a
// plain copy out).  The arena is left unscaled; the peak is read once per tile.
// The aligned / dword split is taken on the destination here.
__global__ __launch_bounds__(kItemThreads, 8) void items_scatter_scaled_kernel(const float *__restrict__ y,
                                                                            const ItemTile *__restrict__ tiles,
                                                                            int64_t ntiles,
                                                                            const ItemFile *__restrict__ files,
                                                                            const ItemSpan *__restrict__ span,
                                                                            const unsigned *__restrict__ peak,
                                                                            int force) {
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const ItemTile tl = tiles[t];
        const Rescale rs = rescale_rule(peak ? __uint_as_float(peak[tl.file]) : 0.0f, force);
        const bool scale = rs.on;
        const double gain = rs.gain;
        const float *__restrict__ src = y + tl.first;
        float *__restrict__ dst = item_span_ptr(tl, files[tl.file], span[tl.file]);
        if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            const float4 *__restrict__ s4 = reinterpret_cast<const float4 *>(src);
            float4 *__restrict__ d4 = reinterpret_cast<float4 *>(dst);
            const int n4 = tl.count >> 2;
            float4 v[kItemLoads];
#pragma unroll
            for (int u = 0; u < kItemLoads; ++u) {
                const int i = (int)threadIdx.x + u * kItemThreads;
                v[u] = i < n4 ? s4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
#pragma unroll
            for (int u = 0; u < kItemLoads; ++u) {
                const int i = (int)threadIdx.x + u * kItemThreads;
                if (i < n4) {
                    if (scale) {
                        v[u].x = scale_one(v[u].x, gain);
                        v[u].y = scale_one(v[u].y, gain);
                        v[u].z = scale_one(v[u].z, gain);
                        v[u].w = scale_one(v[u].w, gain);
                    }
                    d4[i] = v[u];
                }
            }
            const int r = n4 * 4 + (int)threadIdx.x;
            if (r < tl.count) dst[r] = scale ? scale_one(src[r], gain) : src[r];
        } else {
            float v[kItemDwordLoads];
#pragma unroll
            for (int u = 0; u < kItemDwordLoads; ++u) {
                const int i = (int)threadIdx.x + u * kItemThreads;
                v[u] = i < tl.count ? src[i] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < kItemDwordLoads; ++u) {
                const int i = (int)threadIdx.x + u * kItemThreads;
                if (i < tl.count) dst[i] = scale ? scale_one(v[u], gain) : v[u];
            }
        }
    }
}

// decode_pcm_kernel over every file at once: interleaved sample i of file f
// (frame i / nch, channel i % nch) goes to the file's row of that channel.
// Only [0, n_f) of a row is written, so the rows' padding stays zero.
__global__ __launch_bounds__(kItemThreads) void items_decode_kernel(const uint8_t *__restrict__ in,
                                                                    const ItemTile *__restrict__ tiles,
                                                                    int64_t ntiles,
                                                                    const ItemFile *__restrict__ files,
                                                                    const ItemPcm *__restrict__ pcm,
                                                                    float *__restrict__ x) {
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const ItemTile tl = tiles[t];
        const ItemFile fl = files[tl.file];
        const ItemPcm io = pcm[tl.file];
        const uint8_t *__restrict__ src = in + io.byte_off;
        float *__restrict__ dst = x + fl.off;
        uint32_t raw[kItemPcmLoads];
#pragma unroll
        for (int u = 0; u < kItemPcmLoads; ++u) {
            const int k = (int)threadIdx.x + u * kItemThreads;
            if (k < tl.count) raw[u] = load_bytes(src + (tl.first + k) * io.f.bytes, io.f.bytes, io.f.big_endian);
        }
#pragma unroll
        for (int u = 0; u < kItemPcmLoads; ++u) {
            const int k = (int)threadIdx.x + u * kItemThreads;
            if (k < tl.count) {
                const int64_t i = tl.first + k;
                int ch;
                const int64_t fr = split_sample(i, fl.nch, ch);
                dst[(int64_t)ch * fl.stride + fr] = decode_one(raw[u], io.f);
            }
        }
    }
}

// encode_pcm_dither_kernel over every file at once, the one kernel behind
// lcfir_items_encode_pcm_scaled_dev and _dither_dev: file f's decision comes
// from its own peak slot, each sample is scaled as items_normalize_kernel
// would scale it and then encoded; the rows are left unscaled.  ItemTile.first is the
// tile's first interleaved sample of its file, so with frame0 = 0 a sample's
// noise is keyed on its own file's channel and frame: the bytes of a file are
// the per-file call's whatever the batch.  Tiles start a multiple of
// kItemPcmTile samples into the payload, so a tile's quads (two per thread)
// start on dwords exactly where the payload does; such a tile stores dwords
// and its last count % 4 samples bytes, any other keeps the per-sample byte
// store.  peak == nullptr: no rescale.
template <int DITHER>
__global__ __launch_bounds__(kItemThreads) void items_encode_dither_kernel(const float *__restrict__ y,
                                                                           const ItemTile *__restrict__ tiles,
                                                                           int64_t ntiles,
                                                                           const ItemFile *__restrict__ files,
                                                                           const ItemPcm *__restrict__ pcm,
                                                                           const unsigned *__restrict__ peak,
                                                                           int force, uint64_t seed,
                                                                           uint8_t *__restrict__ out) {
    constexpr int kQuads = kItemPcmLoads / 4; // quads per thread and tile
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const ItemTile tl = tiles[t];
        const ItemFile fl = files[tl.file];
        const ItemPcm io = pcm[tl.file];
        const Rescale rs = rescale_rule(peak ? __uint_as_float(peak[tl.file]) : 0.0f, force);
        const bool scale = rs.on;
        const double gain = rs.gain;
        const float *__restrict__ src = y + fl.off;
        uint8_t *__restrict__ dst = out + io.byte_off;
        int done = 0; // samples of the tile the dword path covers
        if ((reinterpret_cast<uintptr_t>(dst + tl.first * io.f.bytes) & 3) == 0) {
            const int vec = quad_vec(src, fl.stride, fl.nch);
            const int nquad = tl.count >> 2;
            float v[kQuads][4];
            int64_t fr[kQuads][4];
            int ch[kQuads][4];
#pragma unroll
            for (int u = 0; u < kQuads; ++u) {
                const int q = (int)threadIdx.x + u * kItemThreads;
                if (q < nquad) load_quad(src, fl.stride, fl.nch, vec, tl.first + 4 * q, v[u], fr[u], ch[u]);
            }
#pragma unroll
            for (int u = 0; u < kQuads; ++u) {
                const int q = (int)threadIdx.x + u * kItemThreads;
                if (q < nquad) {
                    uint32_t e[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float s = scale ? scale_one(v[u][j], gain) : v[u][j];
                        e[j] = encode_one_dither<DITHER>(s, io.f, seed, ch[u][j], (uint64_t)fr[u][j]);
                    }
                    store_quad(dst + (tl.first + 4 * q) * io.f.bytes, e, io.f);
                }
            }
            done = nquad * 4;
        }
        for (int k = done + (int)threadIdx.x; k < tl.count; k += kItemThreads) {
            const int64_t i = tl.first + k;
            int ch;
            const int64_t fr = split_sample(i, fl.nch, ch);
            const float v = src[(int64_t)ch * fl.stride + fr];
            const float s = scale ? scale_one(v, gain) : v;
            store_bytes(dst + i * io.f.bytes, encode_one_dither<DITHER>(s, io.f, seed, ch, (uint64_t)fr), io.f.bytes,
                        io.f.big_endian);
        }
    }
}

} // namespace lcfir
