// Matern-5/2 instances of the mid-width row-weighted gradient product: compiled in parallel with the other kinds
#define CGLB_PREDICT_GRAD_MID_M52
#include "kernels_predict_grad_mid.hip"
