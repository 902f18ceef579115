#define MRA_TU_DIM 3
#define MRA_TU_NAME launch_cascade_d3
#include "mra_launch_prior.inc"
