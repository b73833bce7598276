// Matern-3/2 instances of the mid-width multi-column K_ff product: compiled in parallel with the other kinds
#define CGLB_MULTI_MID_M32
#include "kernels_kff_multi_mid.hip"
