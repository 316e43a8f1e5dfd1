// The per-kernel C entries of libmetro_hip.so (include/metro_hip.h): argument checks in front of a launch_*, plus the
// thread-local error and dispatch-note state every translation unit reports through.
#include <cmath>
#include <cstring>

#include "metro_common.h"

namespace metro {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* get_error() { return g_err; }

static thread_local KernelNotes g_notes = {0, "", {0, 0, 0, 0}};
KernelNotes& kernel_notes() { return g_notes; }
bool note_kernel(const char* fmt, ...) {
    if (g_notes.mode == 0) return false;
    // Mode 1 accumulates until metro_kernel_notes() is called again; an id that does not fit the 4 KiB string is replaced by a
    // trailing " ..." so a truncated string can never pass for an id (a whole metro_forward fits: 45 launches of ResNet-50 are
    // 1.7 KiB, 96 of ResNet-101 3.7 KiB -- tests read the head a forward dispatched from it).
    const size_t cap = sizeof(g_notes.ids) - 5;           // room for " ..."
    const size_t used = strlen(g_notes.ids);
    if (used >= 4 && strcmp(g_notes.ids + used - 4, " ...") == 0) return g_notes.mode == 2;
    char one[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(one, sizeof(one), fmt, ap);
    va_end(ap);
    const size_t need = strlen(one) + (used ? 3 : 0);
    if (used + need > cap) { memcpy(g_notes.ids + used, " ...", 5); return g_notes.mode == 2; }
    if (used) memcpy(g_notes.ids + used, " & ", 3);       // several kernels: a & b
    memcpy(g_notes.ids + used + (used ? 3 : 0), one, strlen(one) + 1);
    return g_notes.mode == 2;
}

int validate_conv_desc(const MetroConvDesc* d) {
    METRO_CHECK_ARG(d != nullptr, "conv desc is NULL");
    METRO_CHECK_ARG(d->n > 0 && d->h_in > 0 && d->w_in > 0 && d->c_in > 0 && d->h_out > 0 &&
                        d->w_out > 0 && d->c_out > 0,
                    "conv desc: non-positive dimension");
    METRO_CHECK_ARG(d->kh > 0 && d->kw > 0 && d->stride > 0 && d->dilation > 0, "conv desc: bad kernel geometry");
    METRO_CHECK_ARG(d->in_pix_stride > 0, "conv desc: in_pix_stride must be positive");
    METRO_CHECK_ARG((long)d->n * d->h_out * d->w_out < (1L << 31), "conv desc: too many output pixels");
    METRO_CHECK_ARG((long)d->n * d->h_in * d->w_in < (1L << 31), "conv desc: too many input pixels");
    if (d->has_prologue) {
        METRO_CHECK_ARG(d->kh == 1 && d->kw == 1, "conv desc: prologue requires a 1x1 kernel");
        const long last_h = (long)(d->h_out - 1) * d->stride - d->pad_top;
        const long last_w = (long)(d->w_out - 1) * d->stride - d->pad_left;
        METRO_CHECK_ARG(d->pad_top <= 0 && d->pad_left <= 0 && last_h < d->h_in && last_w < d->w_in,
                        "conv desc: prologue requires every tap to be in bounds (no padding)");
    }
    if (d->has_residual) {
        METRO_CHECK_ARG(d->res_stride > 0 && d->res_offset >= 0, "conv desc: bad residual gather");
        METRO_CHECK_ARG((d->h_out - 1) * d->res_stride + d->res_offset < d->res_h &&
                            (d->w_out - 1) * d->res_stride + d->res_offset < d->res_w,
                        "conv desc: residual gather out of bounds");
        METRO_CHECK_ARG((long)d->n * d->res_h * d->res_w < (1L << 31), "conv desc: too many residual pixels");
    }
    return METRO_OK;
}

// The conv, stem and head kernels hold PIXEL indices (image x row x column) in int and widen to size_t before the channel count
// goes in: a call fits while its pixel counts fit int32 -- element and byte counts may pass 2^32 (tests/test_gpu_large_address.py).
// The head and stem grids put the image on a grid axis of at most 65 535 blocks.
static int check_image_pixels(const char* who, int32_t n, int32_t side) {
    METRO_CHECK_ARG(side > 0 && (int64_t)n * side * side <= INT32_MAX, "%s: %d images of side %d overflow the int32 pixel index", who, n, side);
    return METRO_OK;
}

}  // namespace metro

using namespace metro;

extern "C" {

int metro_kernel_notes(int32_t mode) {
    METRO_CHECK_ARG(mode >= 0 && mode <= 2, "metro_kernel_notes: mode must be 0 (off), 1 (record) or 2 (dry run)");
    KernelNotes& kn = kernel_notes();
    kn.mode = mode; kn.ids[0] = 0;
    for (int i = 0; i < 4; ++i) kn.schedule[i] = 0;
    return METRO_OK;
}
const char* metro_last_kernel_id(void) { return kernel_notes().ids; }
int metro_last_launch_schedule(int32_t out[4]) {
    METRO_CHECK_ARG(out != nullptr, "metro_last_launch_schedule: out is NULL");
    for (int i = 0; i < 4; ++i) out[i] = kernel_notes().schedule[i];
    return METRO_OK;
}

int metro_conv_f16(const MetroConvDesc* d, const void* d_in, const void* d_w, const float* d_bias,
                   const void* d_pro_scale, const void* d_pro_shift, const void* d_residual,
                   void* d_out, void* stream) {
    int st = validate_conv_desc(d);
    if (st) return st;
    METRO_CHECK_ARG(d->c_in % 8 == 0 && d->in_pix_stride % 4 == 0, "conv_f16: c_in must be a multiple of 8 (got %d) and in_pix_stride of 4", d->c_in);
    METRO_CHECK_ARG(d->c_in <= 2048, "conv_f16: c_in must be <= 2048 (got %d)", d->c_in);
    METRO_CHECK_ARG(d->c_out % 4 == 0, "conv_f16: c_out must be a multiple of 4 (got %d)", d->c_out);
    METRO_CHECK_ARG(d->out_dtype == METRO_F16 || d->out_dtype == METRO_F32, "conv_f16: out_dtype must be F16 or F32");
    METRO_CHECK_ARG(d->in_dtype == METRO_F16, "conv_f16: in_dtype must be F16");
    METRO_CHECK_ARG(!(d->has_residual && d->out_dtype == METRO_F32), "conv_f16: a residual needs F16 output (F32 output has no residual epilogue)");
    METRO_CHECK_ARG(d_in && d_w && d_bias && d_out, "conv_f16: NULL tensor pointer");
    METRO_CHECK_ARG(!d->has_prologue || (d_pro_scale && d_pro_shift), "conv_f16: prologue tensors missing");
    METRO_CHECK_ARG(!d->has_residual || d_residual, "conv_f16: residual tensor missing");
    return launch_conv_f16(*d, {d_in, d_w, d_bias, d_pro_scale, d_pro_shift, d_residual, d_out}, static_cast<hipStream_t>(stream));
}

int metro_conv_f16_pair(const MetroConvDesc* d, const void* d_in, const void* d_w, const float* d_bias,
                        const void* d_pro_scale, const void* d_pro_shift, void* d_out, int32_t split,
                        void* d_out2, void* stream) {
    int st = validate_conv_desc(d);
    if (st) return st;
    METRO_CHECK_ARG(d_in && d_w && d_bias && d_out && d_out2 && d_pro_scale && d_pro_shift, "conv_f16_pair: NULL tensor pointer");
    ConvFused f;
    f.form = ConvForm::Pair;
    f.pair = {split, d->c_out - split, 1, d_out2};
    METRO_CHECK_ARG(conv_form_supported(*d, f), "conv_f16_pair: fp16 1x1 stride-1 convolution with prologue, without residual / ReLU on the "
                    "first output, c_in %% 64; split %d of c_out %d (split %% 256, rest %% 8)", split, d->c_out);
    return launch_conv_f16(*d, {d_in, d_w, d_bias, d_pro_scale, d_pro_shift, nullptr, d_out}, static_cast<hipStream_t>(stream), f);
}

int metro_conv_f16_next(const MetroConvDesc* d, const void* d_in, const void* d_w, const float* d_bias,
                        const void* d_residual, void* d_out, const void* d_w2, const float* d_bias2,
                        const void* d_scale2, const void* d_shift2, void* d_out2, int32_t c2, void* stream) {
    int st = validate_conv_desc(d);
    if (st) return st;
    METRO_CHECK_ARG(d_in && d_w && d_bias && d_out && d_w2 && d_bias2 && d_scale2 && d_shift2 && d_out2,
                    "conv_f16_next: NULL tensor pointer");
    METRO_CHECK_ARG(!d->has_residual || d_residual, "conv_f16_next: residual tensor missing");
    ConvFused f;
    f.form = ConvForm::Next;
    f.next = {d_w2, d_bias2, d_scale2, d_shift2, d_out2, c2};
    METRO_CHECK_ARG(conv_form_supported(*d, f),
                    "conv_f16_next: built for 1x1 stride-1 64 -> 256 with c2 = 64 (block1) and 128 -> 512 with c2 = 128 (block2), fp16");
    return launch_conv_f16(*d, {d_in, d_w, d_bias, nullptr, nullptr, d_residual, d_out}, static_cast<hipStream_t>(stream), f);
}

int metro_conv_f16_conv1_conv2(const MetroConvDesc* d, const void* d_x, const void* d_w1, const float* d_bias1, const void* d_pro_scale,
                               const void* d_pro_shift, const void* d_w2, const float* d_bias2, void* d_out, void* stream) {
    int st = validate_conv_desc(d);
    if (st) return st;
    METRO_CHECK_ARG(d_x && d_w1 && d_bias1 && d_pro_scale && d_pro_shift && d_w2 && d_bias2 && d_out, "conv_f16_conv1_conv2: NULL tensor pointer");
    METRO_CHECK_ARG(conv3x3_c64_supported(*d), "conv_f16_conv1_conv2: built for 3x3 stride-1 SAME 64 -> 64 on maps of <= 64 columns that tile into "
                    "128-pixel row pairs (block1 of the 256-pixel nets)");
    ConvPre1 p1;
    p1.w1 = d_w1; p1.bias1 = d_bias1; p1.pro_scale = d_pro_scale; p1.pro_shift = d_pro_shift;
    return launch_conv3x3_c64(*d, d_x, d_w2, d_bias2, d_out, static_cast<hipStream_t>(stream), &p1);
}

int metro_conv_f16_next_proj(const MetroConvDesc* d, const void* d_in, const void* d_w, const float* d_bias, const void* d_x,
                             const void* d_w_sc, const float* d_bias_sc, const void* d_pro_scale, const void* d_pro_shift, void* d_out,
                             const void* d_w2, const float* d_bias2, const void* d_scale2, const void* d_shift2, void* d_out2,
                             int32_t c2, void* stream) {
    int st = validate_conv_desc(d);
    if (st) return st;
    METRO_CHECK_ARG(d_in && d_w && d_bias && d_x && d_w_sc && d_bias_sc && d_pro_scale && d_pro_shift && d_w2 && d_bias2 &&
                        d_scale2 && d_shift2 && d_out2, "conv_f16_next_proj: NULL tensor pointer");
    ConvFused f;
    f.form = ConvForm::NextProj;
    f.next = {d_w2, d_bias2, d_scale2, d_shift2, d_out2, c2};
    f.psc = {d_x, d_w_sc, d_bias_sc, d_pro_scale, d_pro_shift};
    f.rb.out_mode = d_out == nullptr ? 1 : 0;          // d_out == NULL: the sum stays on chip (it only feeds the second GEMM)
    METRO_CHECK_ARG(conv_form_supported(*d, f), "conv_f16_next_proj: built for 1x1 stride-1 64 -> 256 without prologue / residual, "
                    "c2 = 64 (block1/unit_1), fp16");
    return launch_conv_f16(*d, {d_in, d_w, d_bias, nullptr, nullptr, nullptr, d_out}, static_cast<hipStream_t>(stream), f);
}

int metro_conv_f16_next_rebuild(const MetroConvDesc* d, const void* d_in, const void* d_w, const float* d_bias, const void* d_x,
                                const void* d_w_sc, const float* d_bias_sc, const void* d_pro_scale, const void* d_pro_shift,
                                const void* d_t2_prev, const void* d_w3_prev, const float* d_bias3_prev, void* d_out, void* d_out_sub,
                                int32_t sub_off, const void* d_w2, const float* d_bias2, const void* d_scale2, const void* d_shift2,
                                void* d_out2, int32_t c2, void* stream) {
    int st = validate_conv_desc(d);
    if (st) return st;
    METRO_CHECK_ARG(d_in && d_w && d_bias && d_x && d_w_sc && d_bias_sc && d_pro_scale && d_pro_shift && d_t2_prev && d_w3_prev && d_bias3_prev &&
                        d_w2 && d_bias2 && d_scale2 && d_shift2 && d_out2, "conv_f16_next_rebuild: NULL tensor pointer");
    METRO_CHECK_ARG((d_out != nullptr) != (d_out_sub != nullptr), "conv_f16_next_rebuild: exactly one of d_out (the whole sum) and d_out_sub (its "
                    "sub-sampled compact copy) must be given");
    METRO_CHECK_ARG(sub_off == 0 || sub_off == 1, "conv_f16_next_rebuild: sub_off %d must be 0 or 1", sub_off);
    ConvFused f;
    f.form = ConvForm::NextRebuild;
    f.next = {d_w2, d_bias2, d_scale2, d_shift2, d_out2, c2};
    f.psc = {d_x, d_w_sc, d_bias_sc, d_pro_scale, d_pro_shift};
    ConvRebuild& rb = f.rb;
    rb.t2_prev = d_t2_prev; rb.w3_prev = d_w3_prev; rb.bias3_prev = d_bias3_prev;
    if (d_out_sub != nullptr) {
        rb.out_mode = 2; rb.out_sub = d_out_sub; rb.sub_off = sub_off;
        rb.h_sub = (d->h_out - sub_off + 1) / 2; rb.w_sub = (d->w_out - sub_off + 1) / 2;
    }
    METRO_CHECK_ARG(conv_form_supported(*d, f), "conv_f16_next_rebuild: built for 1x1 stride-1 64 -> 256 without prologue / residual on maps "
                    "whose width is a power of two >= 16 and whose pixel count is a multiple of 64, c2 = 64 (block1/unit_2), fp16");
    return launch_conv_f16(*d, {d_in, d_w, d_bias, nullptr, nullptr, nullptr, d_out}, static_cast<hipStream_t>(stream), f);
}

int metro_conv_b1_form(int32_t classic) {
    METRO_CHECK_ARG(classic == 0 || classic == 1, "metro_conv_b1_form: 0 (default dispatch) or 1 (classic single-role kernel)");
    conv_b1_set_form(classic);
    return METRO_OK;
}

int metro_conv_f16_gemm4w(const MetroConvDesc* d, const void* d_in, const void* d_w, const float* d_bias,
                          const void* d_pro_scale, const void* d_pro_shift, const void* d_residual, void* d_out,
                          int32_t split, void* d_out2, void* stream) {
    int st = validate_conv_desc(d);
    if (st) return st;
    METRO_CHECK_ARG(d_in && d_w && d_bias && d_out, "conv_f16_gemm4w: NULL tensor pointer");
    METRO_CHECK_ARG(!d->has_prologue || (d_pro_scale && d_pro_shift), "conv_f16_gemm4w: prologue tensors missing");
    METRO_CHECK_ARG(!d->has_residual || d_residual, "conv_f16_gemm4w: residual tensor missing");
    METRO_CHECK_ARG(split >= 0 && split < d->c_out && (split == 0 || d_out2), "conv_f16_gemm4w: bad split %d / missing second output", split);
    ConvSplit sp;
    sp.split = split; sp.c_out2 = d->c_out - split; sp.relu2 = 1; sp.out2 = d_out2;
    return launch_conv_gemm4w(*d, {d_in, d_w, d_bias, d_pro_scale, d_pro_shift, d_residual, d_out}, static_cast<hipStream_t>(stream),
                              split > 0 ? &sp : nullptr);
}

int metro_stem_pool_f16(const void* d_prepped, const void* d_w, const float* d_bias, void* d_out, int32_t n,
                        int32_t side, void* stream) {
    METRO_CHECK_ARG(d_prepped && d_w && d_bias && d_out, "stem_pool_f16: NULL tensor pointer");
    METRO_CHECK_ARG(n > 0, "stem_pool_f16: n = %d", n);
    if (const int st = check_image_pixels("stem_pool_f16", n, side)) return st;
    METRO_CHECK_ARG(stem_pool_f16_supported(side, 64), "stem_pool_f16: side %d must be a multiple of 32 (and METRO_STEM_POOL != 0)", side);
    return launch_stem_pool_f16(d_prepped, d_w, d_bias, d_out, n, side, static_cast<hipStream_t>(stream));
}

int metro_stem_pool_f32in(const float* d_images, const void* d_w, const float* d_bias, void* d_out, int32_t n,
                          int32_t side, void* stream) {
    METRO_CHECK_ARG(d_images && d_w && d_bias && d_out, "stem_pool_f32in: NULL tensor pointer");
    METRO_CHECK_ARG(n > 0, "stem_pool_f32in: n = %d", n);
    if (const int st = check_image_pixels("stem_pool_f32in", n, side)) return st;
    METRO_CHECK_ARG(stem_pool_f32in_supported(side, 64), "stem_pool_f32in: side %d must be a multiple of 32 (and METRO_STEM_POOL / METRO_STEM_RAW != 0)", side);
    return launch_stem_pool_f32in(d_images, d_w, d_bias, d_out, n, side, static_cast<hipStream_t>(stream));
}

int metro_stem_pool_u8in(const uint8_t* d_images, const void* d_w, const float* d_bias, void* d_out, int32_t n,
                         int32_t side, void* stream) {
    METRO_CHECK_ARG(d_images && d_w && d_bias && d_out, "stem_pool_u8in: NULL tensor pointer");
    METRO_CHECK_ARG(n > 0, "stem_pool_u8in: n = %d", n);
    if (const int st = check_image_pixels("stem_pool_u8in", n, side)) return st;
    METRO_CHECK_ARG(stem_pool_f32in_supported(side, 64), "stem_pool_u8in: side %d must be a multiple of 32 (and METRO_STEM_POOL / METRO_STEM_RAW != 0)", side);
    return launch_stem_pool_u8in(d_images, d_w, d_bias, d_out, n, side, static_cast<hipStream_t>(stream));
}

int metro_images_u8_to_f32(const uint8_t* d_in, int64_t count, float* d_out, void* stream) {
    METRO_CHECK_ARG(d_in && d_out, "images_u8_to_f32: NULL pointer");
    METRO_CHECK_ARG(count > 0, "images_u8_to_f32: count = %lld", (long long)count);
    return launch_images_u8_to_f32(d_in, (long)count, d_out, static_cast<hipStream_t>(stream));
}

int metro_conv_f64acc(const MetroConvDesc* d, const void* d_in, const double* d_w, const double* d_bias,
                      const double* d_pro_scale, const double* d_pro_shift, const void* d_residual,
                      void* d_out, void* stream) {
    int st = validate_conv_desc(d);
    if (st) return st;
    METRO_CHECK_ARG((d->in_dtype == METRO_F32 || d->in_dtype == METRO_F64) && (d->out_dtype == METRO_F32 || d->out_dtype == METRO_F64) &&
                        !(d->in_dtype == METRO_F64 && d->out_dtype == METRO_F32),
                    "conv_f64acc: in/out dtypes must be F32/F32, F32/F64 or F64/F64");
    METRO_CHECK_ARG(d_in && d_w && d_bias && d_out, "conv_f64acc: NULL tensor pointer");
    METRO_CHECK_ARG(!d->has_prologue || (d_pro_scale && d_pro_shift), "conv_f64acc: prologue tensors missing");
    METRO_CHECK_ARG(!d->has_residual || d_residual, "conv_f64acc: residual tensor missing");
    return launch_conv_f64acc(*d, d_in, d_w, d_bias, d_pro_scale, d_pro_shift, d_residual, d_out,
                              static_cast<hipStream_t>(stream));
}

int metro_conv_f32m(const MetroConvDesc* d, const void* d_in, const float* d_w, const float* d_bias, const float* d_pro_scale,
                    const float* d_pro_shift, const void* d_residual, void* d_out, void* stream) {
    int st = validate_conv_desc(d);
    if (st) return st;
    METRO_CHECK_ARG(d->in_dtype == METRO_F32 && d->out_dtype == METRO_F32, "conv_f32m: in/out dtypes must be F32");
    METRO_CHECK_ARG(d_in && d_w && d_bias && d_out, "conv_f32m: NULL tensor pointer");
    METRO_CHECK_ARG(!d->has_prologue || (d_pro_scale && d_pro_shift), "conv_f32m: prologue tensors missing");
    METRO_CHECK_ARG(!d->has_residual || d_residual, "conv_f32m: residual tensor missing");
    return launch_conv_f32m(*d, d_in, d_w, d_bias, d_pro_scale, d_pro_shift, d_residual, d_out, static_cast<hipStream_t>(stream));
}

int metro_prep_input_f16(const float* d_images, int32_t n, int32_t side, void* d_out, void* stream) {
    METRO_CHECK_ARG(d_images && d_out && n > 0 && side > 0, "prep_input_f16: bad argument");
    return launch_prep_input_f16(d_images, n, side, d_out, static_cast<hipStream_t>(stream));
}

int metro_warp_crop_u8(const uint8_t* d_image, int32_t h, int32_t w, int32_t row_stride, const float* d_homographies,
                       int32_t n, int32_t side, float* d_out, void* stream) {
    METRO_CHECK_ARG(d_image && d_homographies && d_out, "warp_crop_u8: NULL pointer");
    METRO_CHECK_ARG(h > 0 && w > 0 && n > 0 && side > 0 && row_stride >= 3 * w, "warp_crop_u8: bad geometry (h %d w %d stride %d n %d side %d)", h, w, row_stride, n, side);
    METRO_CHECK_ARG(h <= 32767 && w <= 32767, "warp_crop_u8: frames larger than 32767 pixels a side are outside cv2.remap's short coordinates (h %d w %d)", h, w);
    return launch_warp_crop_u8(d_image, h, w, row_stride, d_homographies, d_out, n, side, static_cast<hipStream_t>(stream));
}

}  // extern "C"

// who: the entry's name in its messages; OutT: float crops or the remapped bytes
template <typename OutT>
static int warp_crops_frames_entry(const char* who, const MetroFrame* frames, int32_t n_frames, const MetroCropWarp* d_crops, int32_t n,
                                   int32_t side, OutT* d_out, void* stream) {
    METRO_CHECK_ARG(frames && d_crops && d_out, "%s: NULL pointer", who);
    METRO_CHECK_ARG(n_frames > 0 && n_frames <= METRO_MAX_FRAMES, "%s: %d frames (1 to %d per launch)", who,
                    n_frames, METRO_MAX_FRAMES);
    METRO_CHECK_ARG(n > 0 && side > 0, "%s: bad geometry (n %d side %d)", who, n, side);
    metro::FrameTable table = {};
    for (int i = 0; i < n_frames; ++i) {
        const MetroFrame& f = frames[i];
        METRO_CHECK_ARG(f.data, "%s: frame %d: NULL data pointer", who, i);
        METRO_CHECK_ARG(f.h <= 32767 && f.w <= 32767, "%s: frame %d: frames larger than 32767 pixels a side "
                        "are outside cv2.remap's short coordinates (h %d w %d)", who, i, f.h, f.w);
        METRO_CHECK_ARG(f.h > 0 && f.w > 0 && f.row_stride >= 3 * f.w,
                        "%s: frame %d: bad geometry (h %d w %d stride %d)", who, i, f.h, f.w, f.row_stride);
        table.f[i] = f;
    }
    return launch_warp_crops_frames_u8(table, n_frames, d_crops, n, side, d_out, static_cast<hipStream_t>(stream));
}

template <typename OutT>
static int warp_crops_frames_planes_entry(const char* who, const MetroFramePlanes* frames, int32_t n_frames, const MetroCropWarp* d_crops,
                                          int32_t n, int32_t side, OutT* d_out, void* stream) {
    METRO_CHECK_ARG(frames && d_crops && d_out, "%s: NULL pointer", who);
    METRO_CHECK_ARG(n_frames > 0 && n_frames <= METRO_MAX_FRAMES, "%s: %d frames (1 to %d per launch)", who,
                    n_frames, METRO_MAX_FRAMES);
    METRO_CHECK_ARG(n > 0 && side > 0, "%s: bad geometry (n %d side %d)", who, n, side);
    metro::FramePlanesTable table = {};
    for (int i = 0; i < n_frames; ++i) {
        const MetroFramePlanes& f = frames[i];
        METRO_CHECK_ARG(f.format >= METRO_PIX_RGB && f.format <= METRO_PIX_I420,
                        "%s: frame %d: unknown pixel format %d", who, i, f.format);
        METRO_CHECK_ARG(f.matrix == METRO_YUV_BT601 || f.matrix == METRO_YUV_BT709,
                        "%s: frame %d: unknown colour matrix %d", who, i, f.matrix);
        const bool yuv = f.format == METRO_PIX_NV12 || f.format == METRO_PIX_I420;
        const int n_planes = f.format == METRO_PIX_I420 ? 3 : f.format == METRO_PIX_NV12 ? 2 : 1;
        for (int k = 0; k < n_planes; ++k)
            METRO_CHECK_ARG(f.plane[k], "%s: frame %d: NULL plane %d", who, i, k);
        METRO_CHECK_ARG(f.h > 0 && f.w > 0 && f.h <= 32767 && f.w <= 32767, "%s: frame %d: h %d w %d "
                        "outside [1, 32767] (cv2.remap's short coordinates)", who, i, f.h, f.w);
        METRO_CHECK_ARG(!yuv || (f.h % 2 == 0 && f.w % 2 == 0),
                        "%s: frame %d: 4:2:0 frames need an even h and w (h %d w %d)", who, i, f.h, f.w);
        const int min_stride0 = yuv ? f.w : 3 * f.w;
        METRO_CHECK_ARG(f.stride[0] >= min_stride0, "%s: frame %d: stride[0] %d < %d", who, i, f.stride[0],
                        min_stride0);
        if (yuv) {
            const int min_stride1 = f.format == METRO_PIX_NV12 ? f.w : f.w / 2;
            METRO_CHECK_ARG(f.stride[1] >= min_stride1, "%s: frame %d: stride[1] %d < %d", who, i,
                            f.stride[1], min_stride1);
        }
        table.f[i] = f;
    }
    return launch_warp_crops_frames_planes(table, n_frames, d_crops, n, side, d_out, static_cast<hipStream_t>(stream));
}

extern "C" {

int metro_warp_crops_frames_u8(const MetroFrame* frames, int32_t n_frames, const MetroCropWarp* d_crops, int32_t n,
                               int32_t side, float* d_out, void* stream) {
    return warp_crops_frames_entry("warp_crops_frames_u8", frames, n_frames, d_crops, n, side, d_out, stream);
}

int metro_warp_crops_frames_u8_to_u8(const MetroFrame* frames, int32_t n_frames, const MetroCropWarp* d_crops, int32_t n,
                                     int32_t side, uint8_t* d_out, void* stream) {
    return warp_crops_frames_entry("warp_crops_frames_u8_to_u8", frames, n_frames, d_crops, n, side, d_out, stream);
}

int metro_warp_crops_frames_planes(const MetroFramePlanes* frames, int32_t n_frames, const MetroCropWarp* d_crops,
                                   int32_t n, int32_t side, float* d_out, void* stream) {
    return warp_crops_frames_planes_entry("warp_crops_frames_planes", frames, n_frames, d_crops, n, side, d_out, stream);
}

int metro_warp_crops_frames_planes_to_u8(const MetroFramePlanes* frames, int32_t n_frames, const MetroCropWarp* d_crops,
                                         int32_t n, int32_t side, uint8_t* d_out, void* stream) {
    return warp_crops_frames_planes_entry("warp_crops_frames_planes_to_u8", frames, n_frames, d_crops, n, side, d_out, stream);
}

int metro_eval_metrics(const float* d_pred, const float* d_true, const uint8_t* d_valid, int32_t n, int32_t n_joints,
                       float threshold_mm, float* d_dist, float* d_dist_aligned, double* d_sums, void* stream) {
    METRO_CHECK_ARG(d_pred && d_true && d_valid && d_dist && d_dist_aligned && d_sums, "eval_metrics: NULL pointer");
    METRO_CHECK_ARG(n > 0 && n_joints >= 3 && n_joints <= 1024 && threshold_mm > 0.f, "eval_metrics: bad sizes (n %d, joints %d)", n, n_joints);
    return launch_eval_metrics(d_pred, d_true, d_valid, n, n_joints, threshold_mm, d_dist, d_dist_aligned, d_sums,
                               static_cast<hipStream_t>(stream));
}

int metro_maxpool3x3s2_zeropad(const void* d_in, void* d_out, int32_t n, int32_t h_in, int32_t w_in,
                               int32_t c, int32_t dtype, void* stream) {
    METRO_CHECK_ARG(d_in && d_out && n > 0 && h_in > 0 && w_in > 0 && c > 0, "maxpool: bad argument");
    return launch_maxpool(d_in, d_out, n, h_in, w_in, c, dtype, static_cast<hipStream_t>(stream));
}

int64_t metro_softargmax_scratch_bytes(int32_t n, int32_t side, int32_t n_joints_head) {
    if (n <= 0 || side <= 1 || n_joints_head <= 0) return -1;
    return softargmax_scratch_bytes(n, side, n_joints_head);
}

int metro_softargmax(const void* d_logits, int32_t n, const MetroSpec* spec, int32_t precise,
                     void* d_partials, float* d_poses_out, void* stream) {
    METRO_CHECK_ARG(d_logits && spec && d_partials && d_poses_out && n > 0, "softargmax: bad argument");
    METRO_CHECK_ARG(spec->n_joints_head >= 1 && spec->n_joints_head <= METRO_MAX_JOINTS &&
                        spec->n_joints_out >= 1 && spec->n_joints_out <= METRO_MAX_JOINTS,
                    "softargmax: joint counts out of range");
    METRO_CHECK_ARG(spec->proc_side / spec->stride >= 2, "softargmax: heat-map side must be >= 2");
    const SoftArgmaxArgs a = make_softargmax_args(*spec, n);
    return launch_softargmax(d_logits, a, precise, d_partials, d_poses_out, static_cast<hipStream_t>(stream));
}

int64_t metro_head_f16_scratch_bytes(int32_t n, int32_t side, int32_t n_joints_head) {
    if (n <= 0 || side <= 1 || n_joints_head <= 0) return -1;
    return (int64_t)n * head_f16_slabs(side) * n_joints_head * 5 * (int64_t)sizeof(float);
}

int metro_head_f16(const void* d_x, const void* d_w, const float* d_bias, const void* d_pro_scale, const void* d_pro_shift,
                   int32_t n, int32_t c_in, const MetroSpec* spec, void* d_partials, float* d_logits_out, float* d_poses_out,
                   void* stream) {
    METRO_CHECK_ARG(d_x && d_w && d_bias && d_pro_scale && d_pro_shift && spec && d_partials && d_poses_out && n > 0,
                    "head_f16: bad argument");
    METRO_CHECK_ARG(spec->n_joints_head >= 1 && spec->n_joints_head <= METRO_MAX_JOINTS && spec->n_joints_out >= 1 &&
                        spec->n_joints_out <= METRO_MAX_JOINTS, "head_f16: joint counts out of range");
    METRO_CHECK_ARG((spec->depth * spec->n_joints_head) % 4 == 0, "head_f16: depth*n_joints_head must be a multiple of 4");
    const int side = spec->proc_side / spec->stride;
    if (const int st = check_image_pixels("head_f16", n, side)) return st;
    METRO_CHECK_ARG(n <= 65535, "head_f16: %d images exceed the grid's image axis (65535)", n);
    const SoftArgmaxArgs a = make_softargmax_args(*spec, n);
    int st = launch_head_f16(d_x, d_w, d_bias, d_pro_scale, d_pro_shift, n, c_in, spec->depth * spec->n_joints_head,
                             spec->n_joints_head, spec->depth, side, static_cast<float*>(d_partials), d_logits_out,
                             static_cast<hipStream_t>(stream));
    if (st) return st;
    return launch_softargmax_finalize(static_cast<const float*>(d_partials), a,
                                      head_f16_records(n, c_in, spec->depth * spec->n_joints_head, side), d_poses_out,
                                      static_cast<hipStream_t>(stream));
}

static int check_head_args(const MetroSpec* spec, int32_t n, int32_t n_edges, const char* what);

int metro_head_f16_moments(const void* d_x, const void* d_w, const float* d_bias, const void* d_pro_scale, const void* d_pro_shift,
                           int32_t n, int32_t c_in, const MetroSpec* spec, void* d_partials, void* d_moments_scratch,
                           float* d_logits_out, float* d_poses_out, float* d_coords01_out, float* d_cov01_out, float* d_peak_out,
                           void* stream) {
    METRO_CHECK_ARG(d_x && d_w && d_bias && d_pro_scale && d_pro_shift && spec && d_partials && d_moments_scratch && d_cov01_out &&
                        d_peak_out && n > 0, "head_f16_moments: bad argument");
    METRO_CHECK_ARG(spec->n_joints_head >= 1 && spec->n_joints_head <= METRO_MAX_JOINTS && spec->n_joints_out >= 1 &&
                        spec->n_joints_out <= METRO_MAX_JOINTS, "head_f16_moments: joint counts out of range");
    METRO_CHECK_ARG((spec->depth * spec->n_joints_head) % 4 == 0, "head_f16_moments: depth*n_joints_head must be a multiple of 4");
    const int side = spec->proc_side / spec->stride;
    if (const int st = check_image_pixels("head_f16_moments", n, side)) return st;
    METRO_CHECK_ARG(n <= 65535, "head_f16_moments: %d images exceed the grid's image axis (65535)", n);
    const SoftArgmaxArgs a = make_softargmax_args(*spec, n);
    MomentsOut mo;
    mo.scratch = d_moments_scratch; mo.cov01 = d_cov01_out; mo.peak = d_peak_out;
    int st = launch_head_f16(d_x, d_w, d_bias, d_pro_scale, d_pro_shift, n, c_in, spec->depth * spec->n_joints_head,
                             spec->n_joints_head, spec->depth, side, static_cast<float*>(d_partials), d_logits_out,
                             static_cast<hipStream_t>(stream), static_cast<float*>(d_moments_scratch));
    if (st) return st;
    return launch_softargmax_finalize(static_cast<const float*>(d_partials), a,
                                      head_f16_records(n, c_in, spec->depth * spec->n_joints_head, side), d_poses_out,
                                      static_cast<hipStream_t>(stream), d_coords01_out, nullptr, mo);
}

int metro_softargmax01_moments(const void* d_logits, int32_t n, const MetroSpec* spec, int32_t precise, void* d_partials,
                               void* d_moments_scratch, float* d_coords01_out, float* d_cov01_out, float* d_peak_out,
                               void* stream) {
    METRO_CHECK_ARG(d_logits && spec && d_partials && d_moments_scratch && d_cov01_out && d_peak_out && n > 0,
                    "softargmax01_moments: bad argument");
    METRO_CHECK_ARG(spec->n_joints_head >= 1 && spec->n_joints_head <= METRO_MAX_JOINTS, "softargmax01_moments: joint count out of range");
    METRO_CHECK_ARG(spec->proc_side / spec->stride >= 2, "softargmax01_moments: heat-map side must be >= 2");
    const SoftArgmaxArgs a = make_softargmax_args(*spec, n);
    MomentsOut mo;
    mo.scratch = d_moments_scratch; mo.cov01 = d_cov01_out; mo.peak = d_peak_out;
    return launch_softargmax(d_logits, a, precise, d_partials, nullptr, static_cast<hipStream_t>(stream), d_coords01_out, nullptr, mo);
}

// The three heat-map kernels on the caller's logits: what the bound forwards launch (executor.cpp), with max_n = n.
constexpr int64_t MD_ENTRY_MAX_VOXELS = 64 * 1024;      // one flag byte a voxel: more than the LDS holds
static bool heat_aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }
static int check_heat_args(const char* who, const void* d_logits, int32_t n, const MetroSpec* spec, int32_t precise) {
    METRO_CHECK_ARG(d_logits != nullptr && spec != nullptr, "%s: NULL logits or spec", who);
    METRO_CHECK_ARG(precise >= 0 && precise <= 2, "%s: precise must be 0, 1 or 2 (got %d)", who, precise);
    METRO_CHECK_ARG(heat_aligned(d_logits, precise == 2 ? 8 : 4), "%s: the logits must be aligned to their element", who);
    METRO_CHECK_ARG(n >= 1 && n <= 65535, "%s: %d crops outside [1, 65535] (the grid's crop axis)", who, n);
    METRO_CHECK_ARG(spec->n_joints_head >= 1 && spec->n_joints_head <= METRO_MAX_JOINTS && spec->n_joints_out >= 1 &&
                        spec->n_joints_out <= METRO_MAX_JOINTS, "%s: joint counts out of range (1 to %d)", who, METRO_MAX_JOINTS);
    METRO_CHECK_ARG(spec->depth >= 1 && spec->stride >= 1 && spec->proc_side / spec->stride >= 1,
                    "%s: depth, stride and proc_side / stride must be at least 1", who);
    for (int r = 0; r < spec->n_joints_out; ++r)
        METRO_CHECK_ARG(spec->permutation[r] >= 0 && spec->permutation[r] < spec->n_joints_head,
                        "%s: permutation[%d] = %d is no head joint", who, r, spec->permutation[r]);
    return METRO_OK;
}

int64_t metro_heat_marginals_scratch_bytes(const MetroSpec* spec, int32_t n) {
    if (spec == nullptr || n < 1 || n > 65535 || spec->n_joints_head < 1 || spec->n_joints_head > METRO_MAX_JOINTS || spec->depth < 1 ||
        spec->stride < 1 || spec->proc_side / spec->stride < 1)
        return -1;
    return heat_marginals_scratch_bytes(n, spec->proc_side / spec->stride, spec->n_joints_head, spec->depth, false);
}

int metro_heat_marginals(const void* d_logits, int32_t n, const MetroSpec* spec, int32_t precise, void* d_scratch, float* d_xy_out,
                         float* d_z_out, void* stream) {
    if (const int st = check_heat_args("heat_marginals", d_logits, n, spec, precise)) return st;
    METRO_CHECK_ARG(d_scratch && d_xy_out && d_z_out, "heat_marginals: NULL scratch or output pointer");
    METRO_CHECK_ARG(heat_aligned(d_scratch, 16) && heat_aligned(d_xy_out, 4) && heat_aligned(d_z_out, 4),
                    "heat_marginals: the scratch must be 16-byte and the outputs 4-byte aligned");
    const int side = spec->proc_side / spec->stride;
    METRO_CHECK_ARG((int64_t)side * side <= INT32_MAX / METRO_MAX_JOINTS, "heat_marginals: a map of side %d overflows the int32 row index", side);
    return launch_heat_marginals(d_logits, precise, n, n, *spec, d_scratch, d_xy_out, d_z_out, static_cast<hipStream_t>(stream));
}

int metro_heat_modes(const void* d_logits, int32_t n, const MetroSpec* spec, int32_t precise, int32_t k, int32_t radius,
                     int32_t* d_voxel_out, float* d_stats_out, void* stream) {
    if (const int st = check_heat_args("heat_modes", d_logits, n, spec, precise)) return st;
    METRO_CHECK_ARG(d_voxel_out && d_stats_out, "heat_modes: NULL output pointer");
    METRO_CHECK_ARG(heat_aligned(d_voxel_out, 4) && heat_aligned(d_stats_out, 4), "heat_modes: the outputs must be 4-byte aligned");
    METRO_CHECK_ARG(k >= 1 && k <= METRO_MAX_MODES, "heat_modes: k %d outside [1, %d]", k, METRO_MAX_MODES);
    METRO_CHECK_ARG(radius >= 0 && radius <= METRO_MAX_MODE_RADIUS, "heat_modes: radius %d outside [0, %d]", radius, METRO_MAX_MODE_RADIUS);
    const int side = spec->proc_side / spec->stride;
    if ((int64_t)side * side * spec->depth > MD_ENTRY_MAX_VOXELS) {           // md_flag_bytes in int; no such volume fits the LDS anyway
        set_error("heat_modes: a %d x %d x %d volume does not fit the kernel's LDS", side, side, spec->depth);
        return METRO_ERR_UNSUPPORTED;
    }
    return launch_heat_modes(d_logits, precise, n, n, *spec, k, radius, d_voxel_out, d_stats_out, static_cast<hipStream_t>(stream));
}

int metro_heat_posterior(const void* d_logits, int32_t n, const MetroSpec* spec, int32_t precise, const float* d_prior,
                         float* d_post_out, void* stream) {
    if (const int st = check_heat_args("heat_posterior", d_logits, n, spec, precise)) return st;
    METRO_CHECK_ARG(d_prior && d_post_out, "heat_posterior: NULL prior or output pointer");
    METRO_CHECK_ARG(heat_aligned(d_prior, 4) && heat_aligned(d_post_out, 4), "heat_posterior: the prior and the output must be 4-byte aligned");
    return launch_heat_posterior(d_logits, precise, n, n, *spec, d_prior, d_post_out, static_cast<hipStream_t>(stream));
}

int metro_place_covariances(const float* d_cov01, const float* d_peak, const MetroPlacement* d_records, int32_t n, int32_t n_views,
                            const MetroSpec* spec, const int32_t* d_mirror, int32_t coords, float* d_cov_out, float* d_peak_out,
                            void* stream) {
    int st = check_head_args(spec, n, 0, "place_covariances");
    if (st) return st;
    METRO_CHECK_ARG(coords >= METRO_COORDS_CROP && coords <= METRO_COORDS_WORLD,
                    "place_covariances: coords must be METRO_COORDS_CROP, _CAMERA or _WORLD (got %d)", coords);
    METRO_CHECK_ARG(d_cov01 && d_peak && d_cov_out && d_peak_out, "place_covariances: NULL cov01 / peak / output pointer");
    METRO_CHECK_ARG(coords == METRO_COORDS_CROP || (d_records && d_mirror), "place_covariances: camera / world coords need the records "
                    "and the mirror table");
    METRO_CHECK_ARG(n_views >= 1 && n_views <= METRO_MAX_VIEWS, "place_covariances: %d views (1 to %d)", n_views, METRO_MAX_VIEWS);
    METRO_CHECK_ARG((int64_t)n * n_views * spec->n_joints_head * 6 <= INT32_MAX, "place_covariances: %d boxes x %d views overflow int32",
                    n, n_views);
    return launch_place_covariances(d_cov01, d_peak, d_records, n, n_views, *spec, d_mirror, coords, d_cov_out, d_peak_out,
                                    static_cast<hipStream_t>(stream));
}

int metro_softargmax01(const void* d_logits, int32_t n, const MetroSpec* spec, int32_t precise, void* d_partials,
                       float* d_coords01_out, void* stream) {
    METRO_CHECK_ARG(d_logits && spec && d_partials && d_coords01_out && n > 0, "softargmax01: bad argument");
    METRO_CHECK_ARG(spec->n_joints_head >= 1 && spec->n_joints_head <= METRO_MAX_JOINTS, "softargmax01: joint count out of range");
    METRO_CHECK_ARG(spec->proc_side / spec->stride >= 2, "softargmax01: heat-map side must be >= 2");
    const SoftArgmaxArgs a = make_softargmax_args(*spec, n);
    return launch_softargmax(d_logits, a, precise, d_partials, nullptr, static_cast<hipStream_t>(stream), d_coords01_out);
}

static int check_head_args(const MetroSpec* spec, int32_t n, int32_t n_edges, const char* what) {
    METRO_CHECK_ARG(spec != nullptr && n > 0, "%s: bad argument", what);
    // METRO_MAX_JOINTS is the length of the kernels' per-lane joint and edge arrays (HEAD_MAX, backproject.h)
    METRO_CHECK_ARG(spec->n_joints_head >= 1 && spec->n_joints_head <= METRO_MAX_JOINTS && spec->n_joints_out >= 1 &&
                        spec->n_joints_out <= METRO_MAX_JOINTS, "%s: joint counts out of range (<= %d)", what, METRO_MAX_JOINTS);
    METRO_CHECK_ARG(n_edges >= 0 && n_edges <= METRO_MAX_JOINTS, "%s: at most %d stick-figure edges (got %d)", what,
                    METRO_MAX_JOINTS, n_edges);
    return METRO_OK;
}

int metro_backproject_bone_lengths(const float* d_coords01, const float* d_inv_intrinsics, const double* d_bone_lengths,
                                   int32_t per_pose_lengths, const int32_t* d_edges, int32_t n_edges, int32_t n,
                                   const MetroSpec* spec, int32_t root_relative, int32_t permute, float* d_coords3d_out,
                                   float* d_z_offset_out, void* stream) {
    int st = check_head_args(spec, n, n_edges, "backproject_bone_lengths");
    if (st) return st;
    METRO_CHECK_ARG(d_coords01 && d_inv_intrinsics && d_bone_lengths && d_edges && d_coords3d_out && n_edges >= 1,
                    "backproject_bone_lengths: NULL tensor pointer or no edges");
    return launch_backproject(d_coords01, d_inv_intrinsics, d_bone_lengths, per_pose_lengths != 0, nullptr, d_edges, n,
                              spec->n_joints_head, n_edges, *spec, root_relative, permute, d_coords3d_out, d_z_offset_out,
                              static_cast<hipStream_t>(stream));
}

int metro_backproject_root_depth(const float* d_coords01, const float* d_inv_intrinsics, const float* d_root_z, int32_t n,
                                 const MetroSpec* spec, int32_t root_relative, int32_t permute, float* d_coords3d_out,
                                 void* stream) {
    int st = check_head_args(spec, n, 0, "backproject_root_depth");
    if (st) return st;
    METRO_CHECK_ARG(d_coords01 && d_inv_intrinsics && d_root_z && d_coords3d_out, "backproject_root_depth: NULL tensor pointer");
    return launch_backproject(d_coords01, d_inv_intrinsics, nullptr, 0, d_root_z, nullptr, n, spec->n_joints_head, 0, *spec,
                              root_relative, permute, d_coords3d_out, nullptr, static_cast<hipStream_t>(stream));
}

int metro_heatmap_to_25d(const float* d_coords01, int32_t n, const MetroSpec* spec, float* d_out, void* stream) {
    int st = check_head_args(spec, n, 0, "heatmap_to_25d");
    if (st) return st;
    METRO_CHECK_ARG(d_coords01 && d_out, "heatmap_to_25d: NULL tensor pointer");
    return launch_heatmap_to_25d(d_coords01, d_out, n, *spec, static_cast<hipStream_t>(stream));
}

int metro_to_orig_cam(const float* d_coords, const float* d_rot, const int32_t* d_mirror, float* d_out, int32_t n,
                      int32_t n_joints, void* stream) {
    METRO_CHECK_ARG(d_coords && d_rot && d_mirror && d_out && n > 0 && n_joints >= 1 && n_joints <= METRO_MAX_JOINTS,
                    "to_orig_cam: bad argument (1 <= joints <= %d)", METRO_MAX_JOINTS);
    return launch_to_orig_cam(d_coords, d_rot, d_mirror, d_out, n, n_joints, static_cast<hipStream_t>(stream));
}

int metro_place_poses(const float* d_coords01, const float* d_poses, const MetroPlacement* d_records, int32_t n,
                      const MetroSpec* spec, int32_t scale_recovery, const double* d_bone_lengths, int32_t per_pose_lengths,
                      const float* d_root_depth, const int32_t* d_edges, int32_t n_edges, const int32_t* d_mirror,
                      int32_t coords, float* d_poses_out, float* d_keypoints_out, float* d_z_offset_out, void* stream) {
    const bool bones = scale_recovery == METRO_SCALE_BONE_LENGTHS;
    int st = check_head_args(spec, n, bones ? n_edges : 0, "place_poses");
    if (st) return st;
    METRO_CHECK_ARG(scale_recovery >= METRO_SCALE_METRO && scale_recovery <= METRO_SCALE_TRUE_ROOT_DEPTH,
                    "place_poses: scale_recovery must be METRO_SCALE_METRO, _BONE_LENGTHS or _TRUE_ROOT_DEPTH (got %d)", scale_recovery);
    METRO_CHECK_ARG(coords >= METRO_COORDS_CROP && coords <= METRO_COORDS_WORLD,
                    "place_poses: coords must be METRO_COORDS_CROP, _CAMERA or _WORLD (got %d)", coords);
    METRO_CHECK_ARG(d_coords01 && d_records && d_poses_out && (coords == METRO_COORDS_CROP || d_mirror),
                    "place_poses: NULL coords01 / records / poses_out / mirror pointer");
    METRO_CHECK_ARG(scale_recovery != METRO_SCALE_METRO || d_poses, "place_poses: METRO_SCALE_METRO reads the engine's poses: NULL");
    METRO_CHECK_ARG(!bones || (d_bone_lengths && d_edges && n_edges >= 1), "place_poses: bone-lengths needs lengths and >= 1 edge");
    METRO_CHECK_ARG(scale_recovery != METRO_SCALE_TRUE_ROOT_DEPTH || d_root_depth, "place_poses: true-root-depth needs root depths");
    return launch_place_poses(d_coords01, d_poses, d_records, n, *spec, scale_recovery, d_bone_lengths, per_pose_lengths != 0,
                              d_root_depth, d_edges, bones ? n_edges : 0, d_mirror, coords, d_poses_out, d_keypoints_out,
                              d_z_offset_out, static_cast<hipStream_t>(stream));
}

int metro_expand_views(const MetroViewBase* d_bases, int32_t n, const MetroView* views, int32_t n_views, int32_t side,
                       MetroCropWarp* d_crops_out, MetroPlacement* d_placements_out, void* stream) {
    METRO_CHECK_ARG(d_bases && views && d_crops_out && d_placements_out, "expand_views: NULL pointer");
    METRO_CHECK_ARG(n > 0 && side > 0, "expand_views: bad geometry (n %d side %d)", n, side);
    METRO_CHECK_ARG(n_views >= 1 && n_views <= METRO_MAX_VIEWS, "expand_views: %d views (1 to %d per launch)", n_views,
                    METRO_MAX_VIEWS);
    METRO_CHECK_ARG((int64_t)n * n_views <= INT32_MAX, "expand_views: %d boxes x %d views overflow int32", n, n_views);
    for (int v = 0; v < n_views; ++v) {
        const MetroView& w = views[v];
        METRO_CHECK_ARG(std::isfinite(w.cos_roll) && std::isfinite(w.sin_roll) && std::isfinite(w.zoom) && w.zoom > 0.0,
                        "expand_views: view %d: cos / sin of the roll must be finite and the zoom finite and > 0", v);
        METRO_CHECK_ARG(w.flip == 0 || w.flip == 1, "expand_views: view %d: flip must be 0 or 1 (got %d)", v, w.flip);
    }
    return launch_expand_views(d_bases, n, views, n_views, side, d_crops_out, d_placements_out, static_cast<hipStream_t>(stream));
}

int metro_look_at_boxes(const double* d_boxes, const int32_t* d_frame_index, int32_t n, int32_t n_frames,
                        const MetroFrameCamera* d_cameras, int32_t n_cameras, int32_t side, MetroViewBase* d_bases_out,
                        int32_t* d_status, void* stream) {
    METRO_CHECK_ARG(d_boxes && d_frame_index && d_bases_out && d_status, "look_at_boxes: NULL boxes / frame_index / bases_out / "
                    "status pointer");
    METRO_CHECK_ARG(n > 0 && side > 0, "look_at_boxes: bad geometry (n %d side %d)", n, side);
    METRO_CHECK_ARG(n_frames >= 1 && n_frames <= METRO_MAX_FRAMES, "look_at_boxes: %d frames (1 to %d per launch)", n_frames,
                    METRO_MAX_FRAMES);
    METRO_CHECK_ARG(d_cameras ? (n_cameras == 1 || n_cameras == n_frames) : n_cameras == 0,
                    "look_at_boxes: %d cameras for %d frames (one for every frame, one per frame, or none with a NULL table)",
                    n_cameras, n_frames);
    return launch_look_at_boxes(d_boxes, d_frame_index, n, n_frames, d_cameras, n_cameras, side, d_bases_out, d_status,
                                static_cast<hipStream_t>(stream));
}

int metro_merge_views(const float* d_poses, const float* d_keypoints, const float* d_z_offset, const MetroPlacement* d_records,
                      const int32_t* d_mirror, int32_t n, int32_t n_views, int32_t n_joints, float* d_poses_out,
                      float* d_keypoints_out, float* d_z_offset_out, float* d_spread_out, void* stream) {
    METRO_CHECK_ARG(d_poses && d_poses_out, "merge_views: NULL poses / poses_out pointer");
    METRO_CHECK_ARG(!d_keypoints == !d_keypoints_out, "merge_views: keypoints and keypoints_out go together");
    METRO_CHECK_ARG(!d_z_offset == !d_z_offset_out, "merge_views: z_offset and z_offset_out go together");
    METRO_CHECK_ARG(!d_keypoints || (d_records && d_mirror), "merge_views: keypoints need the records and the mirror table");
    METRO_CHECK_ARG(n > 0 && n_joints >= 1 && n_joints <= METRO_MAX_JOINTS, "merge_views: bad sizes (n %d, joints %d; 1 <= joints <= %d)",
                    n, n_joints, METRO_MAX_JOINTS);
    METRO_CHECK_ARG(n_views >= 1 && n_views <= METRO_MAX_VIEWS, "merge_views: %d views (1 to %d)", n_views, METRO_MAX_VIEWS);
    METRO_CHECK_ARG((int64_t)n * n_views * n_joints * 3 <= INT32_MAX && (int64_t)n * n_joints <= INT32_MAX,
                    "merge_views: %d boxes x %d views overflow int32", n, n_views);
    return launch_merge_views(d_poses, d_keypoints, d_z_offset, d_records, d_mirror, n, n_views, n_joints, d_poses_out,
                              d_keypoints_out, d_z_offset_out, d_spread_out, static_cast<hipStream_t>(stream));
}

// metro_triangulate_joints and metro_triangulate_joints_cov: the second also writes d_cov_out
static int triangulate_joints_entry(const float* d_coords01, const float* d_cov01, const MetroPlacement* d_records, int32_t m,
                                    const int32_t* d_rows, int32_t n_rows, const int32_t* d_starts, int32_t n_persons,
                                    const MetroSpec* spec, const int32_t* d_mirror, int32_t weights, double min_det,
                                    float* d_points_out, int32_t* d_n_rays_out, float* d_residual_out, bool with_cov,
                                    float* d_cov_out, void* stream) {
    METRO_CHECK_ARG(spec != nullptr, "triangulate_joints: NULL spec");
    METRO_CHECK_ARG(spec->n_joints_head >= 1 && spec->n_joints_head <= METRO_MAX_JOINTS && spec->n_joints_out >= 1 &&
                        spec->n_joints_out <= METRO_MAX_JOINTS, "triangulate_joints: joint counts out of range (<= %d)", METRO_MAX_JOINTS);
    METRO_CHECK_ARG(weights == METRO_TRI_UNIFORM || weights == METRO_TRI_COVARIANCE,
                    "triangulate_joints: weights must be METRO_TRI_UNIFORM or METRO_TRI_COVARIANCE (got %d)", weights);
    METRO_CHECK_ARG(n_persons >= 0 && m >= 0 && n_rows >= 0, "triangulate_joints: negative size (persons %d, crop rows %d, "
                    "group rows %d)", n_persons, m, n_rows);
    METRO_CHECK_ARG((int64_t)n_persons * spec->n_joints_out * (with_cov ? 9 : 1) <= INT32_MAX,
                    "triangulate_joints: %d persons overflow int32", n_persons);
    if (n_persons == 0) return METRO_OK;
    METRO_CHECK_ARG(d_starts && d_mirror && d_points_out && d_n_rays_out && d_residual_out,
                    "triangulate_joints: NULL starts / mirror / output pointer");
    METRO_CHECK_ARG(n_rows == 0 || (d_coords01 && d_records && d_rows && m > 0),
                    "triangulate_joints: %d group rows need coords01, records, rows and m > 0", n_rows);
    METRO_CHECK_ARG(weights != METRO_TRI_COVARIANCE || n_rows == 0 || d_cov01,
                    "triangulate_joints: METRO_TRI_COVARIANCE reads cov01: NULL");
    METRO_CHECK_ARG(!with_cov || d_cov_out, "triangulate_joints_cov: NULL cov_out pointer");
    return launch_triangulate_joints(d_coords01, d_cov01, d_records, m, d_rows, n_rows, d_starts, n_persons, *spec, d_mirror, weights,
                                     min_det, d_points_out, d_n_rays_out, d_residual_out, with_cov ? d_cov_out : nullptr,
                                     static_cast<hipStream_t>(stream));
}

int metro_triangulate_joints(const float* d_coords01, const float* d_cov01, const MetroPlacement* d_records, int32_t m,
                             const int32_t* d_rows, int32_t n_rows, const int32_t* d_starts, int32_t n_persons,
                             const MetroSpec* spec, const int32_t* d_mirror, int32_t weights, double min_det, float* d_points_out,
                             int32_t* d_n_rays_out, float* d_residual_out, void* stream) {
    return triangulate_joints_entry(d_coords01, d_cov01, d_records, m, d_rows, n_rows, d_starts, n_persons, spec, d_mirror, weights,
                                    min_det, d_points_out, d_n_rays_out, d_residual_out, false, nullptr, stream);
}

int metro_triangulate_joints_cov(const float* d_coords01, const float* d_cov01, const MetroPlacement* d_records, int32_t m,
                                 const int32_t* d_rows, int32_t n_rows, const int32_t* d_starts, int32_t n_persons,
                                 const MetroSpec* spec, const int32_t* d_mirror, int32_t weights, double min_det,
                                 float* d_points_out, int32_t* d_n_rays_out, float* d_residual_out, float* d_cov_out, void* stream) {
    return triangulate_joints_entry(d_coords01, d_cov01, d_records, m, d_rows, n_rows, d_starts, n_persons, spec, d_mirror, weights,
                                    min_det, d_points_out, d_n_rays_out, d_residual_out, true, d_cov_out, stream);
}

// metro_view_affinity and metro_view_affinity_steps: the second also reads d_step_index
static int view_affinity_entry(const float* d_coords01, const float* d_cov01, const MetroPlacement* d_records, const MetroSpec* spec,
                               const int32_t* d_mirror, const int32_t* d_frame_index, bool with_steps, const int32_t* d_step_index,
                               int32_t n, int32_t n_views, int32_t weights, double min_sin2, double clip_mm, int32_t min_pairs,
                               float* d_cost_out, int32_t* d_n_pairs_out, void* stream) {
    METRO_CHECK_ARG(spec != nullptr, "view_affinity: NULL spec");
    METRO_CHECK_ARG(spec->n_joints_head >= 1 && spec->n_joints_head <= METRO_MAX_JOINTS && spec->n_joints_out >= 1 &&
                        spec->n_joints_out <= METRO_MAX_JOINTS, "view_affinity: joint counts out of range (<= %d)", METRO_MAX_JOINTS);
    METRO_CHECK_ARG(weights == METRO_TRI_UNIFORM || weights == METRO_TRI_COVARIANCE,
                    "view_affinity: weights must be METRO_TRI_UNIFORM or METRO_TRI_COVARIANCE (got %d)", weights);
    METRO_CHECK_ARG(n >= 0, "view_affinity: negative size (%d boxes)", n);
    METRO_CHECK_ARG(n <= METRO_MATCH_MAX_BOXES, "view_affinity: %d boxes (at most %d)", n, METRO_MATCH_MAX_BOXES);
    METRO_CHECK_ARG(n_views >= 1 && n_views <= METRO_MAX_VIEWS, "view_affinity: %d views (1 to %d)", n_views, METRO_MAX_VIEWS);
    METRO_CHECK_ARG(min_sin2 > 0.0 && min_sin2 <= 1.0, "view_affinity: min_sin2 must lie in (0, 1] (got %g)", min_sin2);
    METRO_CHECK_ARG(clip_mm > 0.0, "view_affinity: clip_mm must be > 0 (got %g)", clip_mm);
    METRO_CHECK_ARG(min_pairs >= 1, "view_affinity: min_pairs must be >= 1 (got %d)", min_pairs);
    if (n == 0) return METRO_OK;
    METRO_CHECK_ARG(d_coords01 && d_records && d_mirror && d_frame_index && d_cost_out && d_n_pairs_out,
                    "view_affinity: NULL coords01 / records / mirror / frame_index / output pointer");
    METRO_CHECK_ARG(weights != METRO_TRI_COVARIANCE || d_cov01, "view_affinity: METRO_TRI_COVARIANCE reads cov01: NULL");
    METRO_CHECK_ARG(!with_steps || d_step_index, "view_affinity_steps: NULL step_index pointer");
    return launch_view_affinity(d_coords01, d_cov01, d_records, *spec, d_mirror, d_frame_index, with_steps ? d_step_index : nullptr, n,
                                n_views, weights, min_sin2, clip_mm, min_pairs, d_cost_out, d_n_pairs_out,
                                static_cast<hipStream_t>(stream));
}

int metro_view_affinity(const float* d_coords01, const float* d_cov01, const MetroPlacement* d_records, const MetroSpec* spec,
                        const int32_t* d_mirror, const int32_t* d_frame_index, int32_t n, int32_t n_views, int32_t weights,
                        double min_sin2, double clip_mm, int32_t min_pairs, float* d_cost_out, int32_t* d_n_pairs_out,
                        void* stream) {
    return view_affinity_entry(d_coords01, d_cov01, d_records, spec, d_mirror, d_frame_index, false, nullptr, n, n_views, weights,
                               min_sin2, clip_mm, min_pairs, d_cost_out, d_n_pairs_out, stream);
}

int metro_view_affinity_steps(const float* d_coords01, const float* d_cov01, const MetroPlacement* d_records, const MetroSpec* spec,
                              const int32_t* d_mirror, const int32_t* d_frame_index, const int32_t* d_step_index, int32_t n,
                              int32_t n_views, int32_t weights, double min_sin2, double clip_mm, int32_t min_pairs,
                              float* d_cost_out, int32_t* d_n_pairs_out, void* stream) {
    return view_affinity_entry(d_coords01, d_cov01, d_records, spec, d_mirror, d_frame_index, true, d_step_index, n, n_views, weights,
                               min_sin2, clip_mm, min_pairs, d_cost_out, d_n_pairs_out, stream);
}

int metro_cluster_views(const float* d_cost, int32_t n, int32_t n_views, float max_cost, int32_t* d_person_index_out,
                        int32_t* d_n_persons_out, int32_t* d_rows_out, int32_t* d_starts_out, void* stream) {
    METRO_CHECK_ARG(n >= 0, "cluster_views: negative size (%d boxes)", n);
    METRO_CHECK_ARG(n <= METRO_MATCH_MAX_BOXES, "cluster_views: %d boxes (at most %d)", n, METRO_MATCH_MAX_BOXES);
    METRO_CHECK_ARG(n_views >= 1 && n_views <= METRO_MAX_VIEWS, "cluster_views: %d views (1 to %d)", n_views, METRO_MAX_VIEWS);
    METRO_CHECK_ARG(max_cost > 0.0f, "cluster_views: max_cost must be > 0 (got %g)", (double)max_cost);
    if (n == 0) return METRO_OK;
    METRO_CHECK_ARG(d_cost && d_person_index_out && d_n_persons_out && d_rows_out && d_starts_out,
                    "cluster_views: NULL cost / output pointer");
    return launch_cluster_views(d_cost, n, n_views, max_cost, d_person_index_out, d_n_persons_out, d_rows_out, d_starts_out,
                                static_cast<hipStream_t>(stream));
}

int metro_person_steps(const int32_t* d_rows, int32_t n_rows, const int32_t* d_starts, const int32_t* d_n_persons, int32_t n,
                       int32_t n_views, const int32_t* d_box_step, int32_t n_boxes, const double* d_step_times, int32_t n_steps,
                       int32_t* d_person_step_out, double* d_person_times_out, int32_t* d_step_rows_out, int32_t* d_step_starts_out,
                       void* stream) {
    METRO_CHECK_ARG(n >= 0 && n_rows >= 0 && n_boxes >= 0 && n_steps >= 0,
                    "person_steps: negative size (persons %d, group rows %d, boxes %d, steps %d)", n, n_rows, n_boxes, n_steps);
    METRO_CHECK_ARG(n <= METRO_MATCH_MAX_BOXES, "person_steps: %d persons (at most %d)", n, METRO_MATCH_MAX_BOXES);
    METRO_CHECK_ARG(n_views >= 1 && n_views <= METRO_MAX_VIEWS, "person_steps: %d views (1 to %d)", n_views, METRO_MAX_VIEWS);
    if (n == 0) return METRO_OK;
    METRO_CHECK_ARG(d_starts && d_n_persons && d_person_step_out && d_person_times_out && d_step_rows_out && d_step_starts_out,
                    "person_steps: NULL starts / n_persons / output pointer");
    METRO_CHECK_ARG(n_rows == 0 || (d_rows && d_box_step), "person_steps: %d group rows need rows and box_step", n_rows);
    METRO_CHECK_ARG(n_steps == 0 || d_step_times, "person_steps: %d steps need step_times", n_steps);
    return launch_person_steps(d_rows, n_rows, d_starts, d_n_persons, n, n_views, d_box_step, n_boxes, d_step_times, n_steps,
                               d_person_step_out, d_person_times_out, d_step_rows_out, d_step_starts_out,
                               static_cast<hipStream_t>(stream));
}

int metro_person_steps_labels(const int32_t* d_person_index, const int32_t* d_n_persons, int32_t n, const int32_t* d_box_step,
                              int32_t n_boxes, const double* d_step_times, int32_t n_steps, int32_t* d_person_step_out,
                              double* d_person_times_out, int32_t* d_step_rows_out, int32_t* d_step_starts_out,
                              int32_t* d_single_box_out, void* stream) {
    METRO_CHECK_ARG(n >= 0 && n_boxes >= 0 && n_steps >= 0, "person_steps_labels: negative size (persons %d, boxes %d, steps %d)", n,
                    n_boxes, n_steps);
    METRO_CHECK_ARG(n <= METRO_MATCH_MAX_BOXES, "person_steps_labels: %d persons (at most %d)", n, METRO_MATCH_MAX_BOXES);
    if (n == 0) return METRO_OK;
    METRO_CHECK_ARG(d_n_persons && d_person_step_out && d_person_times_out && d_step_rows_out && d_step_starts_out && d_single_box_out,
                    "person_steps_labels: NULL n_persons / output pointer");
    METRO_CHECK_ARG(n_boxes == 0 || (d_person_index && d_box_step), "person_steps_labels: %d boxes need person_index and box_step",
                    n_boxes);
    METRO_CHECK_ARG(n_steps == 0 || d_step_times, "person_steps_labels: %d steps need step_times", n_steps);
    return launch_person_steps_labels(d_person_index, d_n_persons, n, d_box_step, n_boxes, d_step_times, n_steps, d_person_step_out,
                                      d_person_times_out, d_step_rows_out, d_step_starts_out, d_single_box_out,
                                      static_cast<hipStream_t>(stream));
}

int metro_person_rays(const float* d_coords01, const float* d_cov01, const MetroPlacement* d_records, int32_t m, const MetroSpec* spec,
                      const int32_t* d_mirror, int32_t weights, const int32_t* d_single_box, int32_t n, int32_t n_views,
                      double* d_rays_out, void* stream) {
    METRO_CHECK_ARG(spec != nullptr, "person_rays: NULL spec");
    METRO_CHECK_ARG(spec->n_joints_head >= 1 && spec->n_joints_head <= METRO_MAX_JOINTS && spec->n_joints_out >= 1 &&
                        spec->n_joints_out <= METRO_MAX_JOINTS, "person_rays: joint counts out of range (<= %d)", METRO_MAX_JOINTS);
    METRO_CHECK_ARG(weights == METRO_TRI_UNIFORM || weights == METRO_TRI_COVARIANCE,
                    "person_rays: weights must be METRO_TRI_UNIFORM or METRO_TRI_COVARIANCE (got %d)", weights);
    METRO_CHECK_ARG(n >= 0 && m >= 0, "person_rays: negative size (persons %d, crop rows %d)", n, m);
    METRO_CHECK_ARG(n <= METRO_MATCH_MAX_BOXES, "person_rays: %d persons (at most %d)", n, METRO_MATCH_MAX_BOXES);
    METRO_CHECK_ARG(n_views >= 1 && n_views <= METRO_MAX_VIEWS, "person_rays: %d views (1 to %d)", n_views, METRO_MAX_VIEWS);
    METRO_CHECK_ARG((int64_t)m == (int64_t)n * n_views, "person_rays: %d crop rows are not %d boxes of %d views", m, n, n_views);
    if (n == 0) return METRO_OK;
    METRO_CHECK_ARG(d_coords01 && d_records && d_mirror && d_single_box && d_rays_out,
                    "person_rays: NULL coords01 / records / mirror / single_box / rays_out pointer");
    METRO_CHECK_ARG(weights != METRO_TRI_COVARIANCE || d_cov01, "person_rays: METRO_TRI_COVARIANCE reads cov01: NULL");
    return launch_person_rays(d_coords01, d_cov01, d_records, m, *spec, d_mirror, weights, d_single_box, n, n_views, d_rays_out,
                              static_cast<hipStream_t>(stream));
}

size_t metro_smooth_tracks_workspace_bytes(int32_t n_rows, int32_t n_joints_out) {
    return smooth_tracks_workspace_bytes(n_rows, n_joints_out);
}

int metro_smooth_tracks(const float* d_poses, const float* d_cov, const double* d_times, int32_t n, const int32_t* d_rows,
                        int32_t n_rows, const int32_t* d_starts, int32_t n_tracks, const MetroSpec* spec, int32_t mode,
                        int32_t measurement, double q, double r_floor, double cov_scale, double v0, double gate, double* d_state,
                        void* d_workspace, float* d_poses_out, float* d_velocity_out, float* d_cov_out, uint8_t* d_used_out,
                        void* stream) {
    METRO_CHECK_ARG(spec != nullptr, "smooth_tracks: NULL spec");
    METRO_CHECK_ARG(spec->n_joints_out >= 1 && spec->n_joints_out <= METRO_MAX_JOINTS,
                    "smooth_tracks: n_joints_out %d out of range [1, %d]", spec->n_joints_out, METRO_MAX_JOINTS);
    METRO_CHECK_ARG(mode == METRO_SMOOTH_FILTER || mode == METRO_SMOOTH_RTS,
                    "smooth_tracks: mode must be METRO_SMOOTH_FILTER or METRO_SMOOTH_RTS (got %d)", mode);
    METRO_CHECK_ARG(measurement == METRO_SMOOTH_ISOTROPIC || measurement == METRO_SMOOTH_COVARIANCE,
                    "smooth_tracks: measurement must be METRO_SMOOTH_ISOTROPIC or METRO_SMOOTH_COVARIANCE (got %d)", measurement);
    METRO_CHECK_ARG(n_tracks >= 0 && n >= 0 && n_rows >= 0, "smooth_tracks: negative size (tracks %d, pose rows %d, group rows %d)",
                    n_tracks, n, n_rows);
    METRO_CHECK_ARG(q > 0.0, "smooth_tracks: q must be > 0 (got %g)", q);
    METRO_CHECK_ARG(r_floor > 0.0, "smooth_tracks: r_floor must be > 0 (got %g)", r_floor);
    METRO_CHECK_ARG(v0 > 0.0, "smooth_tracks: v0 must be > 0 (got %g)", v0);
    METRO_CHECK_ARG(cov_scale >= 0.0, "smooth_tracks: cov_scale must be >= 0 (got %g)", cov_scale);
    METRO_CHECK_ARG(gate >= 0.0, "smooth_tracks: gate must be >= 0, 0 for none (got %g)", gate);
    METRO_CHECK_ARG((int64_t)n_tracks * spec->n_joints_out <= INT32_MAX, "smooth_tracks: %d tracks overflow int32", n_tracks);
    if (n_tracks == 0 || n_rows == 0) return METRO_OK;
    METRO_CHECK_ARG(d_poses && d_times && d_rows && d_starts && d_poses_out,
                    "smooth_tracks: NULL poses / times / rows / starts / poses_out pointer");
    METRO_CHECK_ARG(measurement != METRO_SMOOTH_COVARIANCE || d_cov, "smooth_tracks: METRO_SMOOTH_COVARIANCE reads the covariance: NULL");
    METRO_CHECK_ARG(mode != METRO_SMOOTH_RTS || d_workspace, "smooth_tracks: METRO_SMOOTH_RTS needs the workspace: NULL");
    return launch_smooth_tracks(d_poses, d_cov, d_times, n, d_rows, n_rows, d_starts, n_tracks, spec->n_joints_out, mode, measurement,
                                q, r_floor, cov_scale, v0, gate, d_state, d_workspace, d_poses_out, d_velocity_out, d_cov_out,
                                d_used_out, static_cast<hipStream_t>(stream));
}

// The association entries build their record first (make_assoc_args; n_out 0 stands for a NULL spec, which the first check
// below turns away) and check it afterwards.
// The checks of the sizes and numbers that all of them share; r_floor and v0 as given, the record holds their squares.
static int associate_tracks_numbers(const AssocArgs& a, const MetroSpec* spec, double r_floor, double v0) {
    METRO_CHECK_ARG(spec != nullptr, "associate_tracks: NULL spec");
    METRO_CHECK_ARG(spec->n_joints_out >= 1 && spec->n_joints_out <= METRO_MAX_JOINTS,
                    "associate_tracks: n_joints_out %d out of range [1, %d]", spec->n_joints_out, METRO_MAX_JOINTS);
    METRO_CHECK_ARG(a.measurement == METRO_SMOOTH_ISOTROPIC || a.measurement == METRO_SMOOTH_COVARIANCE,
                    "associate_tracks: measurement must be METRO_SMOOTH_ISOTROPIC or METRO_SMOOTH_COVARIANCE (got %d)", a.measurement);
    METRO_CHECK_ARG(a.n >= 0 && a.n_step_rows >= 0 && a.n_steps >= 0,
                    "associate_tracks: negative size (pose rows %d, step rows %d, steps %d)", a.n, a.n_step_rows, a.n_steps);
    METRO_CHECK_ARG(a.n_tracks >= 1 && a.n_tracks <= METRO_ASSOC_MAX, "associate_tracks: %d track slots (1 to %d)", a.n_tracks,
                    METRO_ASSOC_MAX);
    METRO_CHECK_ARG(a.q > 0.0, "associate_tracks: q must be > 0 (got %g)", a.q);
    METRO_CHECK_ARG(r_floor > 0.0, "associate_tracks: r_floor must be > 0 (got %g)", r_floor);
    METRO_CHECK_ARG(v0 > 0.0, "associate_tracks: v0 must be > 0 (got %g)", v0);
    METRO_CHECK_ARG(a.cov_scale >= 0.0, "associate_tracks: cov_scale must be >= 0 (got %g)", a.cov_scale);
    METRO_CHECK_ARG(a.gate >= 0.0, "associate_tracks: gate must be >= 0, 0 for none (got %g)", a.gate);
    METRO_CHECK_ARG(a.max_cost > 0.0f, "associate_tracks: max_cost_mm must be > 0 (got %g)", (double)a.max_cost);
    METRO_CHECK_ARG(a.clip > 0.0, "associate_tracks: clip_mm must be > 0 (got %g)", a.clip);
    METRO_CHECK_ARG(a.max_age >= 0.0, "associate_tracks: max_age_s must be >= 0 (got %g)", a.max_age);
    METRO_CHECK_ARG(a.min_joints >= 1 && a.min_joints <= spec->n_joints_out, "associate_tracks: min_joints %d outside [1, %d]",
                    a.min_joints, spec->n_joints_out);
    return METRO_OK;
}

static bool associate_tracks_nothing_to_do(const AssocArgs& a) { return a.n == 0 || a.n_step_rows == 0 || a.n_steps == 0; }

// every pointer of the record but the covariance
static bool associate_tracks_pointers(const AssocArgs& a) {
    return a.poses && a.times && a.step_rows && a.step_starts && a.state && a.ids && a.next_id && a.ws && a.track_index && a.track_id &&
           a.cost_out && a.rows_out && a.starts_out && a.n_new && a.n_dropped;
}

// the argument checks of both association entries without ray rows, then the launch of one
static int associate_tracks_entry(bool optimal, const AssocArgs& a, const MetroSpec* spec, double r_floor, double v0, void* stream) {
    if (const int rc = associate_tracks_numbers(a, spec, r_floor, v0)) return rc;
    if (associate_tracks_nothing_to_do(a)) return METRO_OK;
    METRO_CHECK_ARG(associate_tracks_pointers(a), "associate_tracks: NULL poses / times / steps / table / workspace / output pointer");
    METRO_CHECK_ARG(a.measurement != METRO_SMOOTH_COVARIANCE || a.cov,
                    "associate_tracks: METRO_SMOOTH_COVARIANCE reads the covariance: NULL");
    return launch_associate_tracks(a, optimal, static_cast<hipStream_t>(stream));
}

size_t metro_associate_tracks_workspace_bytes(int32_t n_tracks, int32_t n_joints_out) {
    return associate_tracks_workspace_bytes(n_tracks, n_joints_out);
}

int metro_associate_tracks(const float* d_poses, const float* d_cov, const double* d_times, int32_t n,
                           const int32_t* d_step_rows, int32_t n_step_rows, const int32_t* d_step_starts, int32_t n_steps,
                           const MetroSpec* spec, int32_t measurement, double q, double r_floor, double cov_scale, double v0,
                           double gate, float max_cost_mm, double clip_mm, int32_t min_joints, double max_age_s, double* d_state,
                           int32_t n_tracks, int32_t* d_ids, int32_t* d_next_id, void* d_workspace, int32_t* d_track_index_out,
                           int32_t* d_track_id_out, float* d_cost_out, int32_t* d_rows_out, int32_t* d_starts_out,
                           int32_t* d_n_new_out, int32_t* d_n_dropped_out, void* stream) {
    const AssocArgs a = make_assoc_args(d_poses, d_cov, d_times, n, d_step_rows, n_step_rows, d_step_starts, n_steps,
                                        spec ? spec->n_joints_out : 0, measurement, q, r_floor, cov_scale, v0, gate, max_cost_mm,
                                        clip_mm, min_joints, max_age_s, d_state, n_tracks, d_ids, d_next_id, d_workspace,
                                        d_track_index_out, d_track_id_out, d_cost_out, d_rows_out, d_starts_out, d_n_new_out,
                                        d_n_dropped_out);
    return associate_tracks_entry(false, a, spec, r_floor, v0, stream);
}

int metro_associate_tracks_optimal(const float* d_poses, const float* d_cov, const double* d_times, int32_t n,
                                   const int32_t* d_step_rows, int32_t n_step_rows, const int32_t* d_step_starts, int32_t n_steps,
                                   const MetroSpec* spec, int32_t measurement, double q, double r_floor, double cov_scale, double v0,
                                   double gate, float max_cost_mm, double clip_mm, int32_t min_joints, double max_age_s, double* d_state,
                                   int32_t n_tracks, int32_t* d_ids, int32_t* d_next_id, void* d_workspace, int32_t* d_track_index_out,
                                   int32_t* d_track_id_out, float* d_cost_out, int32_t* d_rows_out, int32_t* d_starts_out,
                                   int32_t* d_n_new_out, int32_t* d_n_dropped_out, void* stream) {
    const AssocArgs a = make_assoc_args(d_poses, d_cov, d_times, n, d_step_rows, n_step_rows, d_step_starts, n_steps,
                                        spec ? spec->n_joints_out : 0, measurement, q, r_floor, cov_scale, v0, gate, max_cost_mm,
                                        clip_mm, min_joints, max_age_s, d_state, n_tracks, d_ids, d_next_id, d_workspace,
                                        d_track_index_out, d_track_id_out, d_cost_out, d_rows_out, d_starts_out, d_n_new_out,
                                        d_n_dropped_out);
    return associate_tracks_entry(true, a, spec, r_floor, v0, stream);
}

int metro_associate_tracks_rays(float* d_poses, float* d_cov, const double* d_times, int32_t n, const int32_t* d_step_rows,
                                int32_t n_step_rows, const int32_t* d_step_starts, int32_t n_steps, const MetroSpec* spec,
                                int32_t measurement, double q, double r_floor, double cov_scale, double v0, double gate,
                                float max_cost_mm, double clip_mm, int32_t min_joints, double max_age_s, double* d_state,
                                int32_t n_tracks, int32_t* d_ids, int32_t* d_next_id, void* d_workspace, int32_t* d_track_index_out,
                                int32_t* d_track_id_out, float* d_cost_out, int32_t* d_rows_out, int32_t* d_starts_out,
                                int32_t* d_n_new_out, int32_t* d_n_dropped_out, int32_t assignment, const int32_t* d_single_box,
                                const double* d_rays, double depth_sigma_mm, float* d_ray_depth_out, int32_t* d_n_unplaced_out,
                                void* stream) {
    const AssocArgs base = make_assoc_args(d_poses, d_cov, d_times, n, d_step_rows, n_step_rows, d_step_starts, n_steps,
                                           spec ? spec->n_joints_out : 0, measurement, q, r_floor, cov_scale, v0, gate, max_cost_mm,
                                           clip_mm, min_joints, max_age_s, d_state, n_tracks, d_ids, d_next_id, d_workspace,
                                           d_track_index_out, d_track_id_out, d_cost_out, d_rows_out, d_starts_out, d_n_new_out,
                                           d_n_dropped_out);
    const AssocRayArgs a = make_assoc_ray_args(base, d_poses, d_cov, d_single_box, d_rays, depth_sigma_mm, d_ray_depth_out,
                                               d_n_unplaced_out);
    if (const int rc = associate_tracks_numbers(a, spec, r_floor, v0)) return rc;
    METRO_CHECK_ARG(a.measurement == METRO_SMOOTH_COVARIANCE,
                    "associate_tracks_rays: measurement must be METRO_SMOOTH_COVARIANCE (an isotropic R ignores the ray's shape)");
    METRO_CHECK_ARG(assignment == 0 || assignment == 1, "associate_tracks_rays: assignment must be 0 (greedy) or 1 (optimal), got %d",
                    assignment);
    METRO_CHECK_ARG(std::isfinite(depth_sigma_mm) && depth_sigma_mm > 0.0,
                    "associate_tracks_rays: depth_sigma_mm must be finite and > 0 (got %g)", depth_sigma_mm);
    METRO_CHECK_ARG((int64_t)a.n * a.n_out * 9 <= INT32_MAX, "associate_tracks_rays: %d pose rows overflow int32", a.n);
    if (associate_tracks_nothing_to_do(a)) return METRO_OK;
    METRO_CHECK_ARG(associate_tracks_pointers(a) && a.cov,
                    "associate_tracks_rays: NULL poses / cov / times / steps / table / workspace / output pointer");
    METRO_CHECK_ARG(a.single_box && a.rays && a.ray_depth && a.n_unplaced,
                    "associate_tracks_rays: NULL single_box / rays / ray_depth_out / n_unplaced_out pointer");
    return launch_associate_tracks_rays(a, assignment == 1, static_cast<hipStream_t>(stream));
}

int metro_track_bone_lengths(const float* d_poses, const float* d_cov, int32_t n, const int32_t* d_rows, int32_t n_rows,
                             const int32_t* d_starts, int32_t n_tracks, const int32_t* d_ids, int32_t n_joints_out,
                             const int32_t* d_edges, const int32_t* d_edge_mirror, int32_t n_edges, const double* d_fallback,
                             int32_t min_count, double gate, double r_floor, double cov_scale, double min_length_mm, int32_t debias,
                             int32_t symmetric, double* d_stats, int32_t* d_bone_ids, double* d_lengths_out, double* d_sigma_out,
                             uint8_t* d_known_out, void* stream) {
    METRO_CHECK_ARG(n_joints_out >= 1 && n_joints_out <= METRO_MAX_JOINTS, "track_bone_lengths: n_joints_out %d out of range [1, %d]",
                    n_joints_out, METRO_MAX_JOINTS);
    METRO_CHECK_ARG(n_edges >= 1 && n_edges <= METRO_MAX_JOINTS, "track_bone_lengths: %d edges (1 to %d)", n_edges, METRO_MAX_JOINTS);
    METRO_CHECK_ARG(n_tracks >= 1 && n_tracks <= METRO_ASSOC_MAX, "track_bone_lengths: %d track slots (1 to %d)", n_tracks,
                    METRO_ASSOC_MAX);
    METRO_CHECK_ARG(n >= 0 && n_rows >= 0, "track_bone_lengths: negative size (pose rows %d, group rows %d)", n, n_rows);
    METRO_CHECK_ARG(min_count >= 1, "track_bone_lengths: min_count must be >= 1 (got %d)", min_count);
    METRO_CHECK_ARG(gate >= 0.0 && std::isfinite(gate), "track_bone_lengths: gate must be finite and >= 0, 0 for none (got %g)", gate);
    METRO_CHECK_ARG(r_floor > 0.0 && std::isfinite(r_floor), "track_bone_lengths: r_floor must be finite and > 0 (got %g)", r_floor);
    METRO_CHECK_ARG(cov_scale >= 0.0 && std::isfinite(cov_scale), "track_bone_lengths: cov_scale must be finite and >= 0 (got %g)",
                    cov_scale);
    METRO_CHECK_ARG(min_length_mm >= 0.0 && std::isfinite(min_length_mm),
                    "track_bone_lengths: min_length_mm must be finite and >= 0 (got %g)", min_length_mm);
    METRO_CHECK_ARG(d_ids && d_edges && d_edge_mirror && d_stats && d_bone_ids && d_lengths_out && d_sigma_out && d_known_out,
                    "track_bone_lengths: NULL ids / edges / edge_mirror / stats / bone_ids / output pointer");
    METRO_CHECK_ARG(n_rows == 0 || n == 0 || (d_poses && d_rows && d_starts),
                    "track_bone_lengths: %d group rows need poses, rows and starts", n_rows);
    if (n == 0) n_rows = 0;             // no pose row to read: reset and read-out only
    return launch_track_bone_lengths(d_poses, d_cov, n, d_rows, n_rows, d_starts, n_tracks, d_ids, n_joints_out, d_edges, d_edge_mirror,
                                     n_edges, d_fallback, min_count, gate, r_floor, cov_scale, min_length_mm, debias != 0,
                                     symmetric != 0, d_stats, d_bone_ids, d_lengths_out, d_sigma_out, d_known_out,
                                     static_cast<hipStream_t>(stream));
}

const char* metro_last_error(void) { return metro::get_error(); }
int32_t metro_abi_version(void) { return METRO_ABI_VERSION; }

}  // extern "C"
