// spectrum_filter_hi.hip -- the spectral filter's instantiations for log2 N >= 12.
#include "spectrum_dispatch.h"

namespace wsp {

hipError_t launch_spectrum_filter_hi(const SpectrumLaunch &L, hipStream_t stream) {
    return core::dispatch_n_range<double, core::kSetFilter, core::kSplitLog2N, kMaxLog2N>(L, stream);
}

}  // namespace wsp
