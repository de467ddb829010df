// occ/mlp_f16w_occ.hip -- the LIST instantiations of mlp_f16w.hip's forward kernel (the inference forward over the sample list of the
// occupancy-culled render: nh_mlp_forward_f16w_listed), compiled as a translation unit of their own so that the default kernels'
// build time does not grow.
#define NHW_OCC_TU
#include "../mlp_f16w.hip"
