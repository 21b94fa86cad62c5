"""`third_parties.lpips`: the module path the reference's trainer imports (core/train/trainers/occnerf/trainer.py:10,
``from third_parties.lpips import LPIPS``), bound to the gfx950 LPIPS-VGG of occnerf_amd/lpips.py.  With the repository
root on sys.path that import resolves here without an edit, as `_gridencoder` does for the grid encoder."""
from occnerf_amd.lpips import LPIPS, load_vgg16_features, scale_for_lpips  # noqa: F401

__all__ = ['LPIPS', 'load_vgg16_features', 'scale_for_lpips']
