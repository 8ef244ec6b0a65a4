// GMM background kernels (update and segment): Planar frames of two bands, float pixels, 7 to 8 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(float, 2, 7, false);
BG_GMM_LAUNCH(float, 2, 8, false);
