// convert.hip — colour and 16-bit frames to the 8-bit grey plane ahead of the pyramid (contract: include/svo_c.h,
// "pixel formats").  A streaming kernel: a thread owns four adjacent output pixels of one row, cut at the dword
// boundaries of the output so that a whole group is one aligned dword store; it reads its 4, 8, 12 or 16 input bytes
// as aligned dword loads (byte loads where a dword would leave the layout's bytes), and walks its slice of the batch
// the way the remap kernel does.  No LDS.  The body is convert_math.h, shared with the CPU model of the launch.
#include "convert_math.h"
#include "svo_internal.h"

namespace svo {
namespace {

constexpr int kThreads = 256;

struct DeviceMem {
    __device__ __forceinline__ uint32_t ld32(const uint8_t* p) const { return *reinterpret_cast<const uint32_t*>(p); }
    __device__ __forceinline__ uint32_t ld8(const uint8_t* p) const { return *p; }
    __device__ __forceinline__ void st32(uint8_t* p, uint32_t v) const { *reinterpret_cast<uint32_t*>(p) = v; }
    __device__ __forceinline__ void st8(uint8_t* p, uint8_t v) const { *p = v; }
};

template <int kFmt>
__global__ void __launch_bounds__(kThreads)
convert_kernel(ConvertArgs a) {
    DeviceMem mem;
    convert_thread<kFmt>(a, (int64_t)blockIdx.x * kThreads + threadIdx.x, (int32_t)blockIdx.y, mem);
}

template <int kFmt>
void launch(const ConvertArgs& a, hipStream_t s) {
    const uint32_t bx = (uint32_t)(((int64_t)a.groups * a.height + kThreads - 1) / kThreads);
    const uint32_t by = (uint32_t)((a.count + a.per_thread - 1) / a.per_thread);
    hipLaunchKernelGGL(convert_kernel<kFmt>, dim3(bx, by), dim3(kThreads), 0, s, a);
}

}  // namespace

void launch_convert(const ConvertArgs& a, int32_t format, hipStream_t s) {
    if (a.count <= 0 || a.width <= 0 || a.height <= 0) return;
    switch (format) {
        case kPixGray8: launch<kPixGray8>(a, s); break;
        case kPixBgr8: launch<kPixBgr8>(a, s); break;
        case kPixRgb8: launch<kPixRgb8>(a, s); break;
        case kPixBgra8: launch<kPixBgra8>(a, s); break;
        case kPixRgba8: launch<kPixRgba8>(a, s); break;
        case kPixGray16: launch<kPixGray16>(a, s); break;
        default: break;  // (the C ABI rejects any other value before it gets here)
    }
}

}  // namespace svo
