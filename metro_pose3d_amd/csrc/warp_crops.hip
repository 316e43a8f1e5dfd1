// What turns frames and crops into the network's input: input preparation (the stem's bordered fp16 image, uint8 crops) and
// the three crop-warp kernels -- one frame, many packed frames, many frames in several pixel formats (RGB, BGR, NV12, I420).
// No file-scope contraction pragma: the byte path states each rounding through the __f*_rn helpers, and distorted_coords, the
// one NumPy chain in plain operators, states the pragma in its own body.
#include "metro_common.h"
#include "gfx950_prims.h"
#include "camera_math.h"

namespace metro {

// ---------------------------------------------------------------------------------------------
// fp32 NHWC [n,side,side,3] -> fp16 [n,side+6,side+8,4], zero border (3 top/left, 3/5
// bottom/right) and zero 4th channel.  Materialises the stem's explicit pad-3 (reference
// resnet_utils.py:125-135) and the fp32->fp16 cast (architectures.py:29) once, so the 7x7/2
// stem becomes a pad-free 7x1-tap implicit GEMM whose taps are 8 pixels x 4 channels = 32
// contiguous fp16 (the 8th pixel meets zero weights).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_input_f16_kernel(const float* __restrict__ img,
                                                             half4_t* __restrict__ out, int n,
                                                             int side) {
    const int hp = side + 6, wp = side + 8;
    const long total = (long)n * hp * wp;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total;
         p += (long)gridDim.x * blockDim.x) {
        const int x = (int)(p % wp);
        const long t = p / wp;
        const int y = (int)(t % hp);
        const int im = (int)(t / hp);
        half4_t v = {(half_t)0, (half_t)0, (half_t)0, (half_t)0};
        const int yi = y - 3, xi = x - 3;
        if ((unsigned)yi < (unsigned)side && (unsigned)xi < (unsigned)side) {
            const float* s = img + ((size_t)(im * side + yi) * side + xi) * 3;
            v[0] = (half_t)s[0]; v[1] = (half_t)s[1]; v[2] = (half_t)s[2];
        }
        out[p] = v;
    }
}

int launch_prep_input_f16(const float* images, int n, int side, void* out, hipStream_t stream) {
    if (note_kernel("prep_input_f16")) return METRO_OK;
    const long total = (long)n * (side + 6) * (side + 8);
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(prep_input_f16_kernel, dim3(blocks), dim3(256), 0, stream, images,
                       static_cast<half4_t*>(out), n, side);
    return launch_status("prep_input_f16");
}

// ---------------------------------------------------------------------------------------------
// uint8 crops (metro_forward_u8, include/metro_hip.h): byte b stands for the fp32 value fdiv_rn(float(b), 255) clipped to
// [-1, 1] -- normalize01 (reference src/improc.py:56-61), what the crop warp below writes -- and each precision then treats it
// as it treats an fp32 image value.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float u8_unit(unsigned b) { return fminf(fmaxf(__fdiv_rn((float)b, 255.f), -1.f), 1.f); }

// prep_input_f16 from uint8 NHWC [n,side,side,3]: the bits of prep_input_f16 on the fp32 image of the bytes
__global__ __launch_bounds__(256) void prep_input_u8_f16_kernel(const unsigned char* __restrict__ img,
                                                                half4_t* __restrict__ out, int n, int side) {
    const int hp = side + 6, wp = side + 8;
    const long total = (long)n * hp * wp;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total;
         p += (long)gridDim.x * blockDim.x) {
        const int x = (int)(p % wp);
        const long t = p / wp;
        const int y = (int)(t % hp);
        const int im = (int)(t / hp);
        half4_t v = {(half_t)0, (half_t)0, (half_t)0, (half_t)0};
        const int yi = y - 3, xi = x - 3;
        if ((unsigned)yi < (unsigned)side && (unsigned)xi < (unsigned)side) {
            const unsigned char* s = img + ((size_t)(im * side + yi) * side + xi) * 3;
            v[0] = (half_t)u8_unit(s[0]); v[1] = (half_t)u8_unit(s[1]); v[2] = (half_t)u8_unit(s[2]);
        }
        out[p] = v;
    }
}

int launch_prep_input_u8_f16(const unsigned char* images, int n, int side, void* out, hipStream_t stream) {
    if (note_kernel("prep_input_f16<u8in>")) return METRO_OK;
    const long total = (long)n * (side + 6) * (side + 8);
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(prep_input_u8_f16_kernel, dim3(blocks), dim3(256), 0, stream, images,
                       static_cast<half4_t*>(out), n, side);
    return launch_status("prep_input_f16<u8in>");
}

// count bytes -> count fp32 values (metro_images_u8_to_f32): the input of the two parity precisions
__global__ __launch_bounds__(256) void images_u8_to_f32_kernel(const unsigned char* __restrict__ in, float* __restrict__ out,
                                                               long count) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x)
        out[i] = u8_unit(in[i]);
}

int launch_images_u8_to_f32(const unsigned char* in, long count, float* out, hipStream_t stream) {
    if (note_kernel("images_u8_to_f32")) return METRO_OK;
    const int blocks = (int)((count + 255) / 256 < 8192 ? (count + 255) / 256 : 8192);
    hipLaunchKernelGGL(images_u8_to_f32_kernel, dim3(blocks), dim3(256), 0, stream, in, out, count);
    return launch_status("images_u8_to_f32");
}

// ---------------------------------------------------------------------------------------------
// Crop pre-processing (the step BEFORE the path): for every output pixel (x, y) of crop i, source
// coords = H_i * [x, y, 1] (fp32, perspective divide), cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0) of the UINT8 HWC frame, then
// /255 and clip to [-1, 1]: reference src/cameralib.py:406-429 (reproject_image_fast) + src/improc.py:56-61 (normalize01).
// A byte path, reproduced to the byte (oracle/preprocess.py restates the rule from OpenCV's imgwarp.cpp):
//   * coordinates as NumPy's float32 matmul evaluates them: fma(h2, 1, fma(h1, y, rn(h0 * x))), IEEE divide;
//   * OpenCV's fixed point for 8-bit images: s = cvRound(coord * 32) (half to even; NaN / out of int range -> INT_MIN),
//     integer part saturate_cast<short>(s >> 5), 5-bit fractions ax, ay;
//   * 15-bit weights 32 (32 - ay)(32 - ax), 32 (32 - ay) ax, 32 ay (32 - ax), 32 ay ax -- OpenCV's table entry for ax = ay = 0 is
//     (32767, 0, 0, 1) after its sum correction; (32768, 0, 0, 0) gives the same byte for every input since |S11 - S00| < 2^14;
//   * dst = (sum of in-image taps * weights + 2^14) >> 15 (out-of-image taps are the border value 0), a uint8;
//   * normalize01: float(dst) / 255 (IEEE divide), clip.
// One thread per output pixel (3 channels), 12-byte stores.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int cv_round_x86(float v) {
    // cvtss2si: round half to even; NaN and |v| >= 2^31 give the "integer indefinite" INT_MIN
    return (fabsf(v) < 2147483648.f) ? __float2int_rn(v) : (int)0x80000000;
}

// Source coordinates of output pixel (x, y) through homography H (see above).
__device__ __forceinline__ void homography_coords(const float* H, float fx, float fy, float& u, float& v) {
    const float cx = __fmaf_rn(H[2], 1.f, __fmaf_rn(H[1], fy, __fmul_rn(H[0], fx)));
    const float cy = __fmaf_rn(H[5], 1.f, __fmaf_rn(H[4], fy, __fmul_rn(H[3], fx)));
    const float cw = __fmaf_rn(H[8], 1.f, __fmaf_rn(H[7], fy, __fmul_rn(H[6], fx)));
    u = __fdiv_rn(cx, cw);
    v = __fdiv_rn(cy, cw);
}

// One tap's fetch for sample_taps_normalized: adds weight wk times the R, G, B bytes of the in-frame pixel (xx, yy) to
// acc[0..2].  Packed uint8 HWC; BGR reverses the channels on read.
template <bool BGR>
struct PackedFetch {
    const unsigned char* img;
    int row_stride;
    __device__ __forceinline__ void operator()(int xx, int yy, int wk, int acc[3]) const {
        const unsigned char* s = img + (size_t)yy * row_stride + (size_t)xx * 3;
        acc[BGR ? 2 : 0] += wk * (int)s[0]; acc[1] += wk * (int)s[1]; acc[BGR ? 0 : 2] += wk * (int)s[2];
    }
};

// cv2.remap's 8-bit INTER_LINEAR / BORDER_CONSTANT 0 sample at (u, v) of the RGB image whose pixels `fetch` reads, then
// normalize01, into o[0..2] -- or, for uint8 crops (OutT = unsigned char), the remapped byte itself: the value normalize01
// would have divided, which metro_forward_u8 reads by the same rule.  h, w <= 32767: a coordinate saturated to the short range (or INT_MIN >> 5 from a NaN / huge
// value) is outside the frame, and fetch is called for in-frame taps only.
__device__ __forceinline__ void store_sample(float* o, int c, int byte) {
    o[c] = fminf(fmaxf(__fdiv_rn((float)byte, 255.f), -1.f), 1.f);
}
__device__ __forceinline__ void store_sample(unsigned char* o, int c, int byte) { o[c] = (unsigned char)byte; }

template <typename Fetch, typename OutT>
__device__ __forceinline__ void sample_taps_normalized(const Fetch& fetch, int h, int w, float u, float v,
                                                       OutT* __restrict__ o) {
    const int sx = cv_round_x86(__fmul_rn(u, 32.f)), sy = cv_round_x86(__fmul_rn(v, 32.f));
    const int ax = sx & 31, ay = sy & 31;
    int x0 = sx >> 5, y0 = sy >> 5;
    x0 = x0 < -32768 ? -32768 : (x0 > 32767 ? 32767 : x0);          // saturate_cast<short>
    y0 = y0 < -32768 ? -32768 : (y0 > 32767 ? 32767 : y0);
    const int wgt[4] = {32 * (32 - ay) * (32 - ax), 32 * (32 - ay) * ax, 32 * ay * (32 - ax), 32 * ay * ax};
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
        if ((unsigned)xx < (unsigned)w && (unsigned)yy < (unsigned)h) fetch(xx, yy, wgt[k], acc);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int byte = (acc[c] + (1 << 14)) >> 15;                  // <= 255: the weights sum to 2^15
        store_sample(o, c, byte);
    }
}

// The sample of a uint8 HWC RGB frame (row_stride bytes per row).
template <typename OutT>
__device__ __forceinline__ void sample_u8_normalized(const unsigned char* __restrict__ img, int h, int w, int row_stride,
                                                     float u, float v, OutT* __restrict__ o) {
    sample_taps_normalized(PackedFetch<false>{img, row_stride}, h, w, u, v, o);
}

template <typename OutT>
__global__ __launch_bounds__(256) void warp_crop_u8_kernel(const unsigned char* __restrict__ img, int h, int w,
                                                           int row_stride, const float* __restrict__ homs,
                                                           OutT* __restrict__ out, int n, int side) {
    const long total = (long)n * side * side;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const int x = (int)(p % side);
        const long t = p / side;
        const int y = (int)(t % side);
        const int i = (int)(t / side);
        float u, v;
        homography_coords(homs + i * 9, (float)x, (float)y, u, v);
        sample_u8_normalized(img, h, w, row_stride, u, v, out + p * 3);
    }
}

template <typename OutT>
int launch_warp_crop_u8(const unsigned char* img, int h, int w, int row_stride, const float* homs, OutT* out,
                        int n, int side, hipStream_t stream) {
    const long total = (long)n * side * side;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(warp_crop_u8_kernel<OutT>, dim3(blocks), dim3(256), 0, stream, img, h, w, row_stride, homs, out, n, side);
    return launch_status("warp_crop_u8");
}
template int launch_warp_crop_u8<float>(const unsigned char*, int, int, int, const float*, float*, int, int, hipStream_t);
template int launch_warp_crop_u8<unsigned char>(const unsigned char*, int, int, int, const float*, unsigned char*, int, int, hipStream_t);

// ---------------------------------------------------------------------------------------------
// Crops from many frames in one launch (metro_warp_crops_frames_u8, include/metro_hip.h).  Same thread layout and sampling
// as warp_crop_u8_kernel; the crop's record selects the frame and the coordinate chain.  Every lane of a wave reads the same
// record unless the wave straddles two crops (side * side not a multiple of 64).
// DISTORTED: reference cameralib.py:297-312 (fp64 ray of the fp32 grid) and :375-397 (project_points, fp32).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void distorted_coords(const MetroCropWarp& c, float fx, float fy, float& u, float& v) {
    // every product and sum rounded on its own, as NumPy evaluates them: no contraction into fma in this function
    // (plain operators: the pragma does not reach the bodies of the __fmul_rn-style helpers)
#pragma clang fp contract(off)
    const double* P = c.partial;
    const double dx = (double)fx, dy = (double)fy;
    const float rx = (float)((P[0] * dx + P[1] * dy) + P[2]);
    const float ry = (float)((P[3] * dx + P[4] * dy) + P[5]);
    const float rz = (float)((P[6] * dx + P[7] * dy) + P[8]);
    if (!(rz > 0.f)) {                          // behind the camera (or NaN): cv_round_x86(NaN) = INT_MIN -> border
        u = v = __builtin_nanf("");
        return;
    }
    float px = rx / rz, py = ry / rz;
    distort_normalized(c.distortion, px, py);
    const float* K = c.intrinsics;              // K00 K01 K02 K10 K11 K12; [N,2] @ K[:2,:2].T + K[:2,2] like the matmul above
    u = __fmaf_rn(py, K[1], px * K[0]) + K[2];
    v = __fmaf_rn(py, K[4], px * K[3]) + K[5];
}

template <typename OutT>
__global__ __launch_bounds__(256) void warp_crops_frames_u8_kernel(const FrameTable frames, int n_frames,
                                                                   const MetroCropWarp* __restrict__ crops,
                                                                   OutT* __restrict__ out, int n, int side) {
    const long total = (long)n * side * side;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const int x = (int)(p % side);
        const long t = p / side;
        const int y = (int)(t % side);
        const MetroCropWarp& c = crops[t / side];
        const int fi = c.frame;
        OutT* o = out + p * 3;
        if ((unsigned)fi >= (unsigned)n_frames) {
            o[0] = o[1] = o[2] = OutT(0);
            continue;
        }
        const MetroFrame& f = frames.f[fi];
        float u, v;
        if (c.mode == METRO_WARP_DISTORTED)
            distorted_coords(c, (float)x, (float)y, u, v);
        else
            homography_coords(c.homography, (float)x, (float)y, u, v);
        sample_u8_normalized(f.data, f.h, f.w, f.row_stride, u, v, o);
    }
}

template <typename OutT>
int launch_warp_crops_frames_u8(const FrameTable& frames, int n_frames, const MetroCropWarp* crops, int n, int side,
                                OutT* out, hipStream_t stream) {
    const long total = (long)n * side * side;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(warp_crops_frames_u8_kernel<OutT>, dim3(blocks), dim3(256), 0, stream, frames, n_frames, crops, out, n,
                       side);
    return launch_status("warp_crops_frames_u8");
}
template int launch_warp_crops_frames_u8<float>(const FrameTable&, int, const MetroCropWarp*, int, int, float*, hipStream_t);
template int launch_warp_crops_frames_u8<unsigned char>(const FrameTable&, int, const MetroCropWarp*, int, int, unsigned char*, hipStream_t);

// ---------------------------------------------------------------------------------------------
// Crops from frames in several pixel formats in one launch (metro_warp_crops_frames_planes, include/metro_hip.h).  The thread
// layout, both coordinate chains and the remap weights and rounding of warp_crops_frames_u8_kernel; only the per-tap fetch
// differs, chosen per frame (uniform over a wave wherever the wave covers one crop).  A YUV 4:2:0 frame is the RGB image of
// OpenCV's integer cvtColor(COLOR_YUV2RGB_NV12 / _I420) rule (its scalar yuv42xxp2RGB8 path): each in-frame tap reads its Y
// byte and the U, V bytes of its 2x2 block and converts them; out-of-frame taps stay the RGB border 0.
// ---------------------------------------------------------------------------------------------
struct YuvCoeffs { int cy, cvr, cvg, cug, cub; };

// round(c * 2^20) of the three-decimal limited-range coefficients (BT.601: OpenCV's own constants)
__device__ __forceinline__ YuvCoeffs yuv_coeffs(int matrix) {
    return matrix == METRO_YUV_BT709 ? YuvCoeffs{1220542, 1880097, -558891, -223347, 2214593}
                                     : YuvCoeffs{1220542, 1673527, -852492, -409993, 2116026};
}

__device__ __forceinline__ int clamp_u8(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

// NV12 (one interleaved UV plane, the pair read as one 16-bit load) and I420 (separate U and V planes): y_stride / c_stride
// bytes per row.
template <bool NV12>
struct Yuv420Fetch {
    const unsigned char* y;
    const unsigned char* u;
    const unsigned char* v;
    int y_stride, c_stride;
    YuvCoeffs m;
    __device__ __forceinline__ void operator()(int xx, int yy, int wk, int acc[3]) const {
        int cu, cv;
        if (NV12) {
            unsigned short uv;
            __builtin_memcpy(&uv, u + (size_t)(yy >> 1) * c_stride + (size_t)((xx >> 1) * 2), 2);
            cu = (int)(uv & 0xff) - 128;
            cv = (int)(uv >> 8) - 128;
        } else {
            const size_t c = (size_t)(yy >> 1) * c_stride + (size_t)(xx >> 1);
            cu = (int)u[c] - 128;
            cv = (int)v[c] - 128;
        }
        const int ly = (int)y[(size_t)yy * y_stride + xx] - 16;
        const int yv = (ly > 0 ? ly : 0) * m.cy + (1 << 19);       // every intermediate fits in int32
        acc[0] += wk * clamp_u8((yv + m.cvr * cv) >> 20);
        acc[1] += wk * clamp_u8((yv + m.cvg * cv + m.cug * cu) >> 20);
        acc[2] += wk * clamp_u8((yv + m.cub * cu) >> 20);
    }
};

template <typename OutT>
__global__ __launch_bounds__(256) void warp_crops_frames_planes_kernel(const FramePlanesTable frames, int n_frames,
                                                                       const MetroCropWarp* __restrict__ crops,
                                                                       OutT* __restrict__ out, int n, int side) {
    const long total = (long)n * side * side;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const int x = (int)(p % side);
        const long t = p / side;
        const int y = (int)(t % side);
        const MetroCropWarp& c = crops[t / side];
        const int fi = c.frame;
        OutT* o = out + p * 3;
        if ((unsigned)fi >= (unsigned)n_frames) {
            o[0] = o[1] = o[2] = OutT(0);
            continue;
        }
        const MetroFramePlanes& f = frames.f[fi];
        float u, v;
        if (c.mode == METRO_WARP_DISTORTED)
            distorted_coords(c, (float)x, (float)y, u, v);
        else
            homography_coords(c.homography, (float)x, (float)y, u, v);
        if (f.format == METRO_PIX_RGB) {
            sample_taps_normalized(PackedFetch<false>{f.plane[0], f.stride[0]}, f.h, f.w, u, v, o);
        } else if (f.format == METRO_PIX_BGR) {
            sample_taps_normalized(PackedFetch<true>{f.plane[0], f.stride[0]}, f.h, f.w, u, v, o);
        } else if (f.format == METRO_PIX_NV12) {
            const Yuv420Fetch<true> fetch{f.plane[0], f.plane[1], nullptr, f.stride[0], f.stride[1], yuv_coeffs(f.matrix)};
            sample_taps_normalized(fetch, f.h, f.w, u, v, o);
        } else {
            const Yuv420Fetch<false> fetch{f.plane[0], f.plane[1], f.plane[2], f.stride[0], f.stride[1], yuv_coeffs(f.matrix)};
            sample_taps_normalized(fetch, f.h, f.w, u, v, o);
        }
    }
}

template <typename OutT>
int launch_warp_crops_frames_planes(const FramePlanesTable& frames, int n_frames, const MetroCropWarp* crops, int n,
                                    int side, OutT* out, hipStream_t stream) {
    const long total = (long)n * side * side;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(warp_crops_frames_planes_kernel<OutT>, dim3(blocks), dim3(256), 0, stream, frames, n_frames, crops, out,
                       n, side);
    return launch_status("warp_crops_frames_planes");
}
template int launch_warp_crops_frames_planes<float>(const FramePlanesTable&, int, const MetroCropWarp*, int, int, float*, hipStream_t);
template int launch_warp_crops_frames_planes<unsigned char>(const FramePlanesTable&, int, const MetroCropWarp*, int, int, unsigned char*, hipStream_t);

}  // namespace metro
