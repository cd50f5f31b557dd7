// render_chroma.hip — the kRenderChromaUp instantiations of k_render and k_render_scaled (the
// kernels that know bilinear chroma upsampling beside the colour and tone stages) as a code
// object of their own: render.hip's and render_tone.hip's kernels keep their machine code
// byte for byte, and a call without a bilinear image never launches these.
#define HG_RENDER_CHROMA_UNIT 1
#include "render.hip"
