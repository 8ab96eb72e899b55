"""Drop-in for ``arch_search`` (reference arch_search/{evolution,acc_pred,eff_pred}.py, search.py): the evolutionary
search over the supernet's sub-networks, each candidate calibrated and scored on the device.

    python -m litepose_amd.arch_search --cfg supermobile.yaml --supernet supernet.pth --calib-images DIR \\
        --search-images DIR --annotations search.json --constraint 8
"""
from .acc_pred import AccuracyEvaluator  # noqa: F401
from .eff_pred import EfficiencyEvaluator  # noqa: F401
from .evolution import EvolutionFinder  # noqa: F401
