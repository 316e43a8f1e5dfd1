// Which kernel family runs an fp16 convolution.  Host code only, and the only place that knows the order of the families: the
// family files (conv3x3_c64.hip, conv3x3_f16_slab.hip, conv_pws.hip, conv_pw64.hip, conv_b1.hip, conv_gemm4w.hip,
// conv_igemm_f16_dma.hip) each export the predicate and the launcher of their own kernels and never call one another.
#include "metro_common.h"

namespace metro {

bool conv_form_supported(const MetroConvDesc& d, const ConvFused& f) {
    const ConvSplit& s = f.pair;
    const ConvRebuild& rb = f.rb;
    switch (f.form) {
        case ConvForm::Plain:
            return true;          // plain layers: choose_conv_kernel's kernel predicates
        case ConvForm::Pair:      // the ring kernel's pair, which holds every pair conv_pw64 and conv_gemm4w run
            return d.kh == 1 && d.kw == 1 && d.stride == 1 && d.has_prologue && !d.has_residual && !d.relu && d.in_dtype == METRO_F16 &&
                   d.out_dtype == METRO_F16 && d.c_in % 64 == 0 && s.split > 0 && s.c_out2 > 0 && s.split + s.c_out2 == d.c_out &&
                   s.split % 256 == 0 && s.c_out2 % 8 == 0;
        case ConvForm::Next:
            return conv_f16_fuse2_supported(d, f.next.c2) || conv_pw64_supported(d, f);
        case ConvForm::NextProj:  // out_mode 1: the sum only feeds the next conv1 in the launch
            return conv_pw64_supported(d, f) && (rb.out_mode == 0 || rb.out_mode == 1);
        case ConvForm::NextRebuild:   // out_mode 2: only the sub-sampled compact copy of the sum is stored
            return conv_pw64_supported(d, f) &&
                   (rb.out_mode == 0 || (rb.out_mode == 2 && rb.out_sub != nullptr && (rb.sub_off == 0 || rb.sub_off == 1) && rb.h_sub > 0 &&
                                         rb.w_sub > 0));
    }
    return false;
}

// The first family of its form's list whose predicate holds.  Pair and Next have passed conv_form_supported (the planner, the C
// entries), which is what makes the last family of their lists run them.
ConvKernel choose_conv_kernel(const MetroConvDesc& d, const ConvFused& f) {
    switch (f.form) {
        case ConvForm::Plain:
            if (conv3x3_c64_supported(d)) return ConvKernel::C64;
            if (conv3x3_slab_supported(d)) return ConvKernel::Slab;
            if (!conv_f16_dma_supported(d)) return ConvKernel::None;    // the ring kernel's operand rule holds for every family below
            if (conv_pws_supported(d)) return ConvKernel::Pws;
            if (conv_pw64_supported(d, f)) return ConvKernel::Pw64;
            // deep-K pre-activated 1x1 layers with at least one 256 x 256 tile per CU: the four-wave GEMM (128 x 128 wave tiles,
            // register-staged operands, the pre-activation applied once per element on its way into LDS).  Two other forms of this
            // GEMM (8-phase two-wave-group LDS-DMA, round 2; four waves with both operands by LDS-DMA, round 4) give the same bits and
            // measured the same inside the forward: they live in csrc/experimental/ (libmetro_experimental.so), not in the product.
            if (conv_gemm4w_supported(d, nullptr)) return ConvKernel::Gemm4w;
            return ConvKernel::Ring;
        case ConvForm::Pair:
            if (conv_pw64_supported(d, f)) return ConvKernel::Pw64;
            if (conv_gemm4w_supported(d, &f.pair)) return ConvKernel::Gemm4w;
            return ConvKernel::Ring;
        case ConvForm::Next:
            return conv_pw64_supported(d, f) ? ConvKernel::Pw64 : ConvKernel::Fuse2;
        case ConvForm::NextProj:
        case ConvForm::NextRebuild:       // the persistent kernels only
            if (!conv_form_supported(d, f)) return ConvKernel::None;
            return conv_b1_chain_supported(d, f) ? ConvKernel::B1Chain : ConvKernel::Pw64;
    }
    return ConvKernel::None;
}

int launch_conv_f16(const MetroConvDesc& d, const ConvOperands& o, hipStream_t stream, const ConvFused& f) {
    const bool proj = f.form == ConvForm::NextProj || f.form == ConvForm::NextRebuild;
    switch (choose_conv_kernel(d, f)) {
        case ConvKernel::C64: return launch_conv3x3_c64(d, o.in, o.w, o.bias, o.out, stream);
        case ConvKernel::Slab: return launch_conv3x3_slab(d, o.in, o.w, o.bias, o.out, stream);
        case ConvKernel::Pws: return launch_conv_pws(d, o.in, o.w, o.bias, o.residual, o.out, stream);
        case ConvKernel::Pw64:    // a launch with the projection shortcut computed in it has neither a prologue nor a residual tensor
            return launch_conv_pw64(d, proj ? ConvOperands{o.in, o.w, o.bias, nullptr, nullptr, nullptr, o.out} : o, stream, f);
        case ConvKernel::B1Chain: return launch_conv_b1_chain(d, o.in, o.w, o.bias, o.out, stream, f);
        case ConvKernel::Gemm4w: return launch_conv_gemm4w(d, o, stream, f.form == ConvForm::Pair ? &f.pair : nullptr);
        case ConvKernel::Fuse2: return launch_conv_fuse2(d, o, stream, f.next);
        case ConvKernel::Ring: return launch_conv_ring(d, o, stream, f.form == ConvForm::Pair ? &f.pair : nullptr);
        case ConvKernel::None: break;
    }
    if (f.form == ConvForm::Plain)
        set_error("conv_f16: unsupported layer (c_in %d must be a multiple of 8 and <= 2048, in_pix_stride %d of 4 (8 with a "
                  "prologue), c_out %d of 4 (8 with a residual))", d.c_in, d.in_pix_stride, d.c_out);
    else
        set_error("conv_f16: the layer (c_in %d, c_out %d, %d x %d) cannot run in the fused form asked for (conv_form_supported)", d.c_in,
                  d.c_out, d.h_out, d.w_out);
    return METRO_ERR_UNSUPPORTED;
}

}  // namespace metro
