// bk_event_pass.hip -- span_prefix_kernel: at the sample's end, an event pass's `span` prefix-summed in place by one workgroup
// (span_prefix_block, bk_anchor.h).  One kernel for the six passes of bk_event_pass.h; each bk_sample_x launches it once per sample.
#include "bk_event_pass.h"

namespace bk {
namespace {

__global__ __launch_bounds__(kSpanPrefixBlock) void span_prefix_kernel(unsigned int* __restrict__ span, uint32_t n) { span_prefix_block(span, n); }

}  // namespace

void launch_span_prefix(unsigned int* span, uint32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(span_prefix_kernel, dim3(1), dim3(kSpanPrefixBlock), 0, stream, span, n);
}

}  // namespace bk
