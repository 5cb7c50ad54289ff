"""Topological skeletons with UPFlow: `python -m opticalflowscivis_amd.upflow.skeleton --dataset rectangle2d --png-dir shots
--json report.json` traces the separatrices of the saddles of flow_f_out (forward in time) or flow_b_out (backward) on the
device; `--model` is a weights file or a directory holding upflow.pkl; see opticalflowscivis_amd/skeleton.py."""
import sys

from ..skeleton import main_upflow
from .test import Test_model

if __name__ == "__main__":
    main_upflow(Test_model, sys.argv[1:])
