"""UPFlow test (UPFlow/test.py): `Test_model.eval_forward` and `scivis_test`, which scores the forward and backward
flows against the known motion of a sequence instead of only printing them (the reference's
"EPE All / F1 / EPE Noc / EPE Occ" lines are commented out there):

    python -m opticalflowscivis_amd.upflow.test --dataset rectangle2d --gap 1 --zero-baseline --out result.json

`--model` is a weights file or a directory holding upflow.pkl; see opticalflowscivis_amd/flow_eval.py."""
import os
import sys

import torch

from ..flow_eval import main_upflow
from .model.upflow import UPFlow_net


class Test_model:
    """UPFlow/test.py:107-152: the network as the reference tests it (normalised cost volume, self-guided
    up-sampling), in eval mode on the GPU."""

    def __init__(self, pretrain_path="train_log/upflow.pkl"):
        conf = UPFlow_net.config()
        conf.update({"if_norm_before_cost_volume": True, "norm_moments_across_channels": False,
                     "norm_moments_across_images": False, "if_froze_pwc": False, "if_sgu_upsample": True})
        net = conf()
        path = pretrain_path
        if os.path.isdir(path):
            path = os.path.join(path, "upflow.pkl")
        if os.path.exists(path):
            net.load_model(path, if_relax=True, if_print=True)
        else:
            print("no upflow.pkl under %s: using random-init weights" % pretrain_path)
        self.net_work = net.to(torch.device("cuda")).eval()

    def __call__(self, input_dict):
        return self.net_work(input_dict)

    def eval_forward(self, im1, im2):
        """The forward flow im1 -> im2 (UPFlow/test.py:131-143)."""
        with torch.no_grad():
            return self.net_work({"im1": im1, "im2": im2, "if_loss": False})["flow_f_out"]


def scivis_test(argv=None):
    """Score flow_f_out of (t, t+gap) and flow_b_out of (t+gap, t) on a sequence with known motion."""
    return main_upflow(Test_model, argv)


if __name__ == "__main__":
    scivis_test(sys.argv[1:])
