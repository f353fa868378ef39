// nfp_tile_r3_fwd.hip — the radius-3 (k = 7) instantiations of the row-band forward, a unit of their own: the launcher of
// nfp_tile_fwd.hip compiled for R = 3 alone (interface: nfp_launch.h::tile_forward_r3, which tile_forward hands g.R == 3 to).
#define NFP_TILE_R3_UNIT 1
#include "nfp_tile_fwd.hip"
