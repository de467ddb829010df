// occ/mlp16_occ.hip -- the LIST instantiations of mlp16.hip's forward kernel (the inference forward over the sample list of the
// occupancy-culled render: nh_mlp16_forward_listed), widths 64 / 128 / 256, compiled as a translation unit of their own so that the
// default kernels' build time does not grow.
#define NH16_OCC_TU
#include "../mlp16.hip"
