// resample_tone.hip — the tone instantiations of k_render_resampled (kRenderTone), a code
// object of their own as render_tone.hip is: resample.hip's kernels keep their machine code.
#define HG_RENDER_TONE_UNIT 1
#include "resample.hip"
