"""Vortex regions with UPFlow: `python -m opticalflowscivis_amd.upflow.regions --dataset rectangle2d --json report.json`
labels the vortex regions of flow_f_out (forward in time) or flow_b_out (backward), measures them, links them along the
flow and reports tracks and events; `--model` is a weights file or a directory holding upflow.pkl; see
opticalflowscivis_amd/regions.py."""
import sys

from ..regions import main_upflow
from .test import Test_model

if __name__ == "__main__":
    main_upflow(Test_model, sys.argv[1:])
