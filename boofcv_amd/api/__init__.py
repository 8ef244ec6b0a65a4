"""Host-side mirror of the reference's interfaces, on top of the C ABI: one module per family of include/boofhip.h and csrc/cabi_*.hip.

Names, argument meaning and error behaviour follow the Java reference (waicool20/BoofCV 0.35-SNAPSHOT) so that the parity
tests read like the reference's own tests; every call runs hand-written HIP kernels in libboofhip.so on an MI355X.

    F: = main/boofcv-feature/src/main/java/boofcv/   I: = main/boofcv-ip/src/main/java/boofcv/   T: = main/boofcv-types/src/main/java/boofcv/

Imports run one way: core <- image <- every family; detect <- surf, klt, template; filter <- surf; klt <- flow; distort <- background.
Every public name of every module is re-exported here (`api.X`), with the private helpers device.py, sharded.py and the tests use.
"""
from . import associate, background, core, detect, disparity, distort, filter, flow, image, klt, surf, template
from .associate import *  # noqa: F401,F403
from .background import *  # noqa: F401,F403
from .core import *  # noqa: F401,F403
from .core import _check, _NativeObject, _PinnedPool  # noqa: F401  (device.py, sharded.py and the tests)
from .detect import *  # noqa: F401,F403
from .disparity import *  # noqa: F401,F403
from .distort import *  # noqa: F401,F403
from .distort import _host_map, _kernel_model  # noqa: F401  (tests)
from .filter import *  # noqa: F401,F403
from .flow import *  # noqa: F401,F403
from .image import *  # noqa: F401,F403
from .klt import *  # noqa: F401,F403
from .klt import _klt_fetch  # noqa: F401  (device.py)
from .surf import *  # noqa: F401,F403
from .template import *  # noqa: F401,F403

__all__ = sum((m.__all__ for m in (core, image, associate, detect, filter, surf, klt, disparity, template, distort, background, flow)), [])
