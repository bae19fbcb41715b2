// The transducer beam search (rnnt_beam.hip) on a stateless predictor: the
// RT_PRED_CTX instantiations of rnnt_beam_kernel, with and without an LM, and
// their launch.  They are compiled here, apart from the LSTM instantiations,
// so that the object of rnnt_beam.hip stays what it was and this one is built
// without packed fp32 instructions (rt_ctx_gather's adds stay scalar, one
// rounding per written operation, as in the greedy kernel of
// rnnt_stateless.hip: beam 1 equals that kernel bit for bit).
#define ASR_RNNT_BEAM_KERNEL_ONLY
#include "rnnt_beam.hip"

namespace asr {

int rnnt_beam_ctx_launch(const BeamArgs& a, const BeamLmArgs& q, bool lm, unsigned tiles, size_t lds, hipStream_t st) {
    if (lm) {
        static AsrAttrOnce attr;
        if (int rc = attr.set((const void*)rnnt_beam_kernel<true, RT_PRED_CTX>, RT_LDS_MAX)) return rc;
        hipLaunchKernelGGL((rnnt_beam_kernel<true, RT_PRED_CTX>), dim3(tiles), dim3(64 * RT_WAVES), lds, st, a, q);
    } else {
        static AsrAttrOnce attr;
        if (int rc = attr.set((const void*)rnnt_beam_kernel<false, RT_PRED_CTX>, RT_LDS_MAX)) return rc;
        hipLaunchKernelGGL((rnnt_beam_kernel<false, RT_PRED_CTX>), dim3(tiles), dim3(64 * RT_WAVES), lds, st, a, q);
    }
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // namespace asr
