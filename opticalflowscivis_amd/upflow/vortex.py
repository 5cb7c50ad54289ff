"""Vortex and divergence fields with UPFlow: `python -m opticalflowscivis_amd.upflow.vortex --dataset rectangle2d --json
report.json` differentiates flow_f_out (forward in time) or flow_b_out (backward) into divergence, vorticity, Q and
lambda2 on the device; `--model` is a weights file or a directory holding upflow.pkl; see
opticalflowscivis_amd/vortex.py."""
import sys

from ..vortex import main_upflow
from .test import Test_model

if __name__ == "__main__":
    main_upflow(Test_model, sys.argv[1:])
