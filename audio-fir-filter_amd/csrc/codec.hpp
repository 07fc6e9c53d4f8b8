// codec.hpp -- on-device sample codec either side of the hot path
// (SURVEY.md s8f row 1).
//
// The reference reads a whole file into a deinterleaved AudioBuffer of
// VectorMath<float32_t> (AudioSamples::readAll, ProcessFile.cp:40-41) and
// writes it back with AudioSamples::writeAll(buf, true) (:115-117); both live
// in the un-vendored c_lib, so the exact scaling/rounding is parity-unpinned.
// We use the standard conventions:
//   decode  int b-bit  v -> (float) v / 2^(b-1)        (exact in f32 for b <= 24)
//           float32    v -> v
//   encode  float f -> clamp(rint(f * 2^(b-1)), -2^(b-1), 2^(b-1) - 1)  (RNE, in f64)
//           float32    f -> f
// Interleaved frames (WAV: little-endian, AIFF: big-endian) <-> planar
// channels [nch][frames] with a channel stride, byte-exact, no MFMA:
//   decode_pcm_kernel         one thread per interleaved sample, byte loads;
//   encode_pcm_dither_kernel  the one encode kernel behind lcfir_encode_pcm_dev,
//                             _scaled_dev and _dither_dev: four samples a lane,
//                             whole dwords stored where d_out allows, the
//                             normalize (peak_scale.hpp's rule) folded in and
//                             the dither a template parameter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcfir {

struct PcmFormat {
    int bytes;      // 2, 3, 4
    bool is_float;  // float32 (bytes == 4)
    bool big_endian;
};

__device__ __forceinline__ uint32_t load_bytes(const uint8_t *__restrict__ p, int nb, bool be) {
    uint32_t v = 0;
    if (be) {
        for (int b = 0; b < nb; ++b) v = (v << 8) | p[b];
    } else {
        for (int b = nb - 1; b >= 0; --b) v = (v << 8) | p[b];
    }
    return v;
}

__device__ __forceinline__ void store_bytes(uint8_t *__restrict__ p, uint32_t v, int nb, bool be) {
    if (be) {
        for (int b = nb - 1; b >= 0; --b) {
            p[b] = (uint8_t)(v & 0xff);
            v >>= 8;
        }
    } else {
        for (int b = 0; b < nb; ++b) {
            p[b] = (uint8_t)(v & 0xff);
            v >>= 8;
        }
    }
}

__device__ __forceinline__ float decode_one(uint32_t raw, const PcmFormat f) {
    if (f.is_float) return __uint_as_float(raw);
    const int bits = 8 * f.bytes;
    const int32_t s = (int32_t)(raw << (32 - bits)) >> (32 - bits); // sign-extend
    return (float)((double)s * (1.0 / (double)(1u << (bits - 1))));
}

__device__ __forceinline__ uint32_t encode_one(float v, const PcmFormat f) {
    if (f.is_float) return __float_as_uint(v);
    const int bits = 8 * f.bytes;
    const double scale = (double)(1ull << (bits - 1));
    double q = rint((double)v * scale);
    const double lo = -scale, hi = scale - 1.0;
    q = q < lo ? lo : (q > hi ? hi : q);
    if (q != q) q = 0.0; // NaN -> 0
    return (uint32_t)(int32_t)(int64_t)q;
}

// Interleaved sample i = frame * nch + ch: its frame, and its channel in ch.
__device__ __forceinline__ int64_t split_sample(int64_t i, int nch, int &ch) {
    const int64_t fr = i / nch;
    ch = (int)(i - fr * nch);
    return fr;
}

// grid-stride over the interleaved sample index
__global__ __launch_bounds__(256) void decode_pcm_kernel(const uint8_t *__restrict__ in, PcmFormat f,
                                                        int nch, int64_t frames,
                                                        float *__restrict__ out, int64_t stride) {
    const int64_t total = frames * nch;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        int ch;
        const int64_t fr = split_sample(i, nch, ch);
        const uint32_t raw = load_bytes(in + i * f.bytes, f.bytes, f.big_endian);
        out[(int64_t)ch * stride + fr] = decode_one(raw, f);
    }
}

// ---- TPDF dither (include/lcfir.h, LCFIR_DITHER_TPDF) --------------------------
// The noise is a pure function of (seed, channel, absolute frame index of the
// file), so the bytes of a file do not depend on how its frames were cut into
// calls, launches, devices or item-set rows: a splitmix64 finaliser over a
// per-channel stream, the difference of its two 32-bit halves as a triangular
// variate in (-1, 1) LSB.  Every step is exact (integers modulo 2^64, two
// u32 -> f64 conversions, one exact subtraction, a power-of-two scaling), so
// host and device agree to the bit and a numpy restatement can pin the bytes.
constexpr int kDitherNone = 0;
constexpr int kDitherTpdf = 1;

__host__ __device__ __forceinline__ uint64_t dither_hash(uint64_t seed, int32_t ch, uint64_t frame) {
    const uint64_t s = seed ^ ((uint64_t)(ch + 1) * 0xD1B54A32D192ED03ull);
    uint64_t z = s + frame * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__host__ __device__ __forceinline__ double dither_tpdf(uint64_t seed, int32_t ch, uint64_t frame) {
    const uint64_t z = dither_hash(seed, ch, frame);
    return ((double)(uint32_t)(z >> 32) - (double)(uint32_t)z) * (1.0 / 4294967296.0);
}

// encode_one with the noise added before the rounding: the product is a
// power-of-two scaling of an f32, hence exact, so the add is the only f64
// rounding and contracting it into an fma changes nothing.  Float formats
// pass their bits through, dither or not.
template <int DITHER>
__device__ __forceinline__ uint32_t encode_one_dither(float v, const PcmFormat f, uint64_t seed, int32_t ch,
                                                      uint64_t frame) {
    if (DITHER == kDitherNone || f.is_float) return encode_one(v, f);
    const int bits = 8 * f.bytes;
    const double scale = (double)(1ull << (bits - 1));
    double q = rint((double)v * scale + dither_tpdf(seed, ch, frame));
    const double lo = -scale, hi = scale - 1.0;
    q = q < lo ? lo : (q > hi ? hi : q);
    if (q != q) q = 0.0; // NaN -> 0
    return (uint32_t)(int32_t)(int64_t)q;
}

// Four consecutive interleaved samples [i0, i0 + 4) of a planar block: their
// values, channels and frames.  One 64-bit division per quad; the rest steps.
// vec 1: one channel, 16-byte aligned row -> one float4; vec 2: two channels,
// 8-byte aligned rows -> two float2; vec 0: four loads, each lane walking its
// rows in step with its neighbours (lane l + 1 is four samples on).
__device__ __forceinline__ void load_quad(const float *__restrict__ in, int64_t stride, int nch, int vec,
                                          int64_t i0, float v[4], int64_t fr[4], int ch[4]) {
    if (nch == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fr[j] = i0 + j;
            ch[j] = 0;
        }
        if (vec == 1) {
            const float4 a = *reinterpret_cast<const float4 *>(in + i0);
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = in[i0 + j];
        }
    } else if (nch == 2) {
        const int64_t f0 = i0 >> 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fr[j] = f0 + (j >> 1);
            ch[j] = j & 1;
        }
        if (vec == 2) {
            const float2 a = *reinterpret_cast<const float2 *>(in + f0);
            const float2 b = *reinterpret_cast<const float2 *>(in + stride + f0);
            v[0] = a.x, v[1] = b.x, v[2] = a.y, v[3] = b.y;
        } else {
            v[0] = in[f0], v[1] = in[stride + f0], v[2] = in[f0 + 1], v[3] = in[stride + f0 + 1];
        }
    } else {
        int64_t f = i0 / nch;
        int c = (int)(i0 - f * nch);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fr[j] = f;
            ch[j] = c;
            v[j] = in[(int64_t)c * stride + f];
            if (++c == nch) c = 0, ++f;
        }
    }
}

// Which of load_quad's forms a block of rows allows (wave-uniform).
__device__ __forceinline__ int quad_vec(const float *in, int64_t stride, int nch) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(in);
    if (nch == 1) return (a & 15) == 0 ? 1 : 0;
    if (nch == 2) return (a & 7) == 0 && (stride & 1) == 0 ? 2 : 0;
    return 0;
}

// 2, 3 and 4 dwords that need dword alignment only: one global_store_dwordx2
// / x3 / x4 each (gfx950 takes them at any dword address).
typedef uint32_t dwords2 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t dwords3 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t dwords4 __attribute__((ext_vector_type(4), aligned(4)));

// Four encoded samples as the 2, 3 or 4 dwords of their 8, 12 or 16 bytes
// in the stream, in one store.  p must be 4-byte aligned.
__device__ __forceinline__ void store_quad(uint8_t *__restrict__ p, const uint32_t e[4], const PcmFormat f) {
    uint32_t s[4]; // the sample as the little-endian value of its stream bytes
#pragma unroll
    for (int j = 0; j < 4; ++j)
        s[j] = f.big_endian ? __builtin_bswap32(e[j]) >> (32 - 8 * f.bytes)
                            : (f.bytes == 4 ? e[j] : e[j] & ((1u << (8 * f.bytes)) - 1u));
    if (f.bytes == 2) {
        dwords2 w = {s[0] | (s[1] << 16), s[2] | (s[3] << 16)};
        *reinterpret_cast<dwords2 *>(p) = w;
    } else if (f.bytes == 3) {
        dwords3 w = {s[0] | (s[1] << 24), (s[1] >> 8) | (s[2] << 16), (s[2] >> 16) | (s[3] << 8)};
        *reinterpret_cast<dwords3 *>(p) = w;
    } else {
        dwords4 w = {s[0], s[1], s[2], s[3]};
        *reinterpret_cast<dwords4 *>(p) = w;
    }
}

// The encode, with ProcessFile.cp:91-101's normalize folded in: the per-file
// decision (peak = max d_peak[0..npeak), rescale_rule) is read from the
// device, and each sample is scaled exactly as normalize_kernel does before
// it is encoded -- byte-identical to normalize + encode, without the rescale
// pass's 8 B/sample of HBM traffic; npeak = 0 is the plain encode.
// A lane produces four consecutive interleaved samples; where d_out is
// 4-byte aligned every quad starts on a dword (4 * bytes per quad), so the
// quads go out as dwords and only the buffer's last total % 4 samples as
// bytes.  An unaligned d_out takes one byte store per sample throughout.  The
// test is on a kernel argument, hence wave-uniform (items_gather_kernel's
// float4 split).  Sample i of the call is frame frame0 + i / nch of its file
// (kDitherNone uses neither seed nor frame0).
template <int DITHER>
__global__ __launch_bounds__(256) void encode_pcm_dither_kernel(const float *__restrict__ in, int64_t stride,
                                                               int nch, int64_t frames, PcmFormat f,
                                                               const unsigned *__restrict__ peak, int npeak,
                                                               int force, uint64_t seed, uint64_t frame0,
                                                               uint8_t *__restrict__ out) {
    float pk = 0.0f;
    for (int i = 0; i < npeak; ++i) pk = fmaxf(pk, __uint_as_float(peak[i]));
    // rescale_rule (peak_scale.hpp) spelled out: through the helper the compiler turns two branches round
    const bool scale = (pk > 1.0f || force) && pk > 0.0f;
    const double gain = scale ? 1.0 / (double)pk : 1.0;
    const int64_t total = frames * nch;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0; // samples the dword path covers
    if ((reinterpret_cast<uintptr_t>(out) & 3) == 0) {
        const int vec = quad_vec(in, stride, nch);
        const int64_t nquad = total >> 2;
        for (int64_t q = tid; q < nquad; q += nthreads) {
            float v[4];
            int64_t fr[4];
            int ch[4];
            uint32_t e[4];
            load_quad(in, stride, nch, vec, q * 4, v, fr, ch);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (scale) v[j] = (float)((double)v[j] * gain);
                e[j] = encode_one_dither<DITHER>(v[j], f, seed, ch[j], frame0 + (uint64_t)fr[j]);
            }
            store_quad(out + q * 4 * f.bytes, e, f);
        }
        done = nquad * 4;
    }
    for (int64_t i = done + tid; i < total; i += nthreads) {
        int ch;
        const int64_t fr = split_sample(i, nch, ch);
        float v = in[(int64_t)ch * stride + fr];
        if (scale) v = (float)((double)v * gain);
        store_bytes(out + i * f.bytes, encode_one_dither<DITHER>(v, f, seed, ch, frame0 + (uint64_t)fr), f.bytes,
                    f.big_endian);
    }
}

} // namespace lcfir
