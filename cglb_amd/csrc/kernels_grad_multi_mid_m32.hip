// Matern-3/2 instances of the mid-width multi-pair gradient pass: compiled in parallel with the other kinds
#define CGLB_GRAD_MULTI_MID_M32
#include "kernels_grad_multi_mid.hip"
