// The one launch sequence of every kernel, for HIP translation units: the raw launch macro appears here and nowhere else (tests/test_host.py).
#pragma once
#include <optional>
#include <utility>

#include "common.h"

namespace fc {

// Launches Kern under a profile scope named prof_name (the name rocprofv3 prints; null: an unprofiled launch) and checks the launch.
// A scope that spans several launches stays with its caller, which launches with a null name inside it.
// MAX_LDS: the most dynamic LDS any launch of Kern asks for; above 64 KB the kernel's limit is raised to it once per device (the template
// argument gives every kernel its own PerDeviceOnce).  At the default 0 a launch is the scope, the launch and the check, nothing else.
template <auto Kern>
PerDeviceOnce& kernel_attr_once() {
    static PerDeviceOnce once;
    return once;
}
template <auto Kern, int MAX_LDS = 0, class... Args>
void launch_kernel(const char* prof_name, double flops, double bytes, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args&&... args) {
    if constexpr (MAX_LDS > 65536) {
        kernel_attr_once<Kern>().run([](int) { FC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS)); return 0; });
    }
    std::optional<ProfScope> ps;
    if (prof_name) ps.emplace(prof_name, flops, bytes, s);
    hipLaunchKernelGGL(Kern, grid, block, lds, s, std::forward<Args>(args)...);
    FC_HIP(hipGetLastError());
}

}  // namespace fc
