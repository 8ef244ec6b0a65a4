// GMM background kernels (update and segment): Planar frames of one band, float pixels, 1 to 6 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(float, 1, 1, false);
BG_GMM_LAUNCH(float, 1, 2, false);
BG_GMM_LAUNCH(float, 1, 3, false);
BG_GMM_LAUNCH(float, 1, 4, false);
BG_GMM_LAUNCH(float, 1, 5, false);
BG_GMM_LAUNCH(float, 1, 6, false);
