"""reftr_amd — MI355X-native (gfx950) implementation of the RefTR training hot path.

Public surface mirrors the reference (ubc-vision/RefTR) Python protocol; see INTEGRATION.md:
    from reftr_amd import build_reftr                      # models/__init__.py:4
    from reftr_amd.engine_vg import train_one_epoch, evaluate
    from reftr_amd.optim import build_optimizer
    from reftr_amd.parallel import DistributedDataParallel
    from reftr_amd import Predictor                        # raw images + phrases -> boxes and original-size masks (predict.py)
    from reftr_amd import evaluate_raw                     # evaluate() for a loader of raw batches, on a batch canvas (engine_vg.py)
"""
__version__ = "0.1.0"

from .models import build_reftr  # noqa: E402,F401
from .predict import Predictor  # noqa: E402,F401
from .engine_vg import evaluate_raw  # noqa: E402,F401
