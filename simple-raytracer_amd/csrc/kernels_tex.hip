// kernels_tex.hip -- the textured twins of the trace kernel and the denoiser's feature kernels: the text of kernels.hip with
// SRT_TEXTURED set (see the note at the top of that file and DESIGN.md §13). A translation unit of its own, so that the
// untextured kernels are compiled from exactly the text they were compiled from before albedo textures existed.
#define SRT_TEXTURED 1
#include "kernels.hip"
