// nfp_tile_r3_bwd.hip — the radius-3 (k = 7) instantiations of the row-band backward, a unit of their own: the launcher of
// nfp_tile_bwd.hip compiled for R = 3 alone (interface: nfp_launch.h::tile_backward_r3, which tile_backward hands g.R == 3 to).
#define NFP_TILE_R3_UNIT 1
#include "nfp_tile_bwd.hip"
