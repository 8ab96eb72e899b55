"""Drop-in for ``models.pose_simplenet`` (reference lib/models/pose_simplenet.py).

pose_simplenet is LitePose without the Fusion Deconv Head: the same stem, InvBottleneck stages and head geometry, but
each deconv layer is ``ConvTranspose2d(refined) -> BN -> ReLU`` and each output stage is ``final_refined[i-1]`` alone
(pose_simplenet.py:128-136).  The wrapper is ``models.pose_mobilenet.LitePose`` with ``lp_arch.plain_head = 1``: its
``state_dict()`` keys are the reference module's (no ``deconv_raw.*`` / ``final_raw.*``) and a strict
``load_state_dict`` refuses a pose_mobilenet checkpoint.
"""
from . import pose_mobilenet as _pm


class LitePose(_pm.LitePose):
    def __init__(self, cfg, width_mult=1.0, round_nearest=8, cfg_arch=None, storage=None):
        """``storage``: see ``models.pose_mobilenet.LitePose``."""
        super(LitePose, self).__init__(cfg, width_mult, round_nearest, cfg_arch=cfg_arch, storage=storage,
                                       plain_head=True)


def get_pose_net(cfg, is_train=False, cfg_arch=None, storage=None):
    """pose_simplenet.py:138-156.  As in models.pose_mobilenet, pre-trained backbone loading (is_train and
    INIT_WEIGHTS) is a training feature and out of scope: weights arrive through ``load_state_dict``."""
    return LitePose(cfg, cfg_arch=cfg_arch, storage=storage)
