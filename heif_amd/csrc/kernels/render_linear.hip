// render_linear.hip — the kRenderLinear instantiations of k_render_scaled (the area average taken
// in linear light: in_lut before the sum, matrix and out_lut behind the quotient) as a code
// object of their own: the kernels of render.hip, render_tone.hip and render_chroma.hip keep
// their machine code byte for byte, and a call without the option never launches these.
#define HG_RENDER_LINEAR_UNIT 1
#include "render.hip"
