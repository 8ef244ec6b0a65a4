// GMM background kernels (update and segment): GrayF32 frames, 1 to 6 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(float, 1, 1, true);
BG_GMM_LAUNCH(float, 1, 2, true);
BG_GMM_LAUNCH(float, 1, 3, true);
BG_GMM_LAUNCH(float, 1, 4, true);
BG_GMM_LAUNCH(float, 1, 5, true);
BG_GMM_LAUNCH(float, 1, 6, true);
