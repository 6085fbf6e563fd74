"""``pytorch_msssim`` as the reference's evaluation code imports it (trainer.py:38, test.py:34): ``ssim``, ``ms_ssim``, ``SSIM`` and
``MS_SSIM`` with pytorch_msssim's names, argument order and defaults, on the MI355X kernels (``3d-magic-mirror_amd/ssim.py``).

Kept apart from ``shim/`` so that putting ``shim/`` on ``sys.path`` never hides a pytorch_msssim that is already installed; opting in is
a second line:

    sys.path.insert(0, "<repo>/3d-magic-mirror_amd/shim_eval")
"""
import importlib
import os
import sys

_ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
if _ROOT not in sys.path:
    sys.path.append(_ROOT)                                       # behind the caller's own entries, as in shim/kaolin/_mm.py

_impl = importlib.import_module("3d-magic-mirror_amd.ssim")
ssim = _impl.ssim
ms_ssim = _impl.ms_ssim
SSIM = _impl.SSIM
MS_SSIM = _impl.MS_SSIM

__all__ = ["ssim", "ms_ssim", "SSIM", "MS_SSIM"]
__version__ = "1.0.0+mi355x"
