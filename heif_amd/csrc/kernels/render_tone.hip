// render_tone.hip — the tone instantiations of k_render and k_render_scaled (kRenderTone:
// the colour-managed kernels that also know the tone stage of an HDR source) as a code
// object of their own: render.hip's kernels keep their machine code byte for byte.
#define HG_RENDER_TONE_UNIT 1
#include "render.hip"
