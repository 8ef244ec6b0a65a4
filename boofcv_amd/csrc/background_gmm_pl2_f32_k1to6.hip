// GMM background kernels (update and segment): Planar frames of two bands, float pixels, 1 to 6 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(float, 2, 1, false);
BG_GMM_LAUNCH(float, 2, 2, false);
BG_GMM_LAUNCH(float, 2, 3, false);
BG_GMM_LAUNCH(float, 2, 4, false);
BG_GMM_LAUNCH(float, 2, 5, false);
BG_GMM_LAUNCH(float, 2, 6, false);
