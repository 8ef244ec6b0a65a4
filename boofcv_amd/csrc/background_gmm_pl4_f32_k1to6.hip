// GMM background kernels (update and segment): Planar frames of four bands, float pixels, 1 to 6 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(float, 4, 1, false);
BG_GMM_LAUNCH(float, 4, 2, false);
BG_GMM_LAUNCH(float, 4, 3, false);
BG_GMM_LAUNCH(float, 4, 4, false);
BG_GMM_LAUNCH(float, 4, 5, false);
BG_GMM_LAUNCH(float, 4, 6, false);
