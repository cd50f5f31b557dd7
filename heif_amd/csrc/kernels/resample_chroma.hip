// resample_chroma.hip — the kRenderChromaUp instantiations of k_render_resampled as a code
// object of their own (as render_chroma.hip): resample.hip's kernels keep their machine code.
#define HG_RENDER_CHROMA_UNIT 1
#include "resample.hip"
