// spectrum_filter.hip -- the fused spectral band-pass (forward FFT, real mask over the packed elements,
// inverse or last sample + peak: the per-bar pipeline of L/WaveSpecZZ_1.0.4-core.mq5:561-578) as two more
// outputs of the spectrum kernel, fp64, log2 N < 12; log2 N >= 12 in spectrum_filter_hi.hip.
#include "spectrum_dispatch.h"

namespace wsp {

hipError_t launch_spectrum_filter(const SpectrumLaunch &L, hipStream_t stream) {
    if (L.f32 || !L.mask || (L.output != kOutFiltSeries && L.output != kOutFiltLast)) return hipErrorInvalidValue;
    if (L.log2n >= core::kSplitLog2N) return launch_spectrum_filter_hi(L, stream);
    return core::dispatch_n_range<double, core::kSetFilter, 5, core::kSplitLog2N - 1>(L, stream);
}

}  // namespace wsp
