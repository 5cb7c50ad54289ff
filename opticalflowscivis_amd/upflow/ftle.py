"""FTLE fields with UPFlow: `python -m opticalflowscivis_amd.upflow.ftle --dataset rectangle2d --window 2 --json
report.json` advects a lattice through flow_f_out (forward in time) or flow_b_out (backward) and reduces the flow map to
Lyapunov exponents; `--model` is a weights file or a directory holding upflow.pkl; see opticalflowscivis_amd/ftle.py."""
import sys

from ..ftle import main_upflow
from .test import Test_model

if __name__ == "__main__":
    main_upflow(Test_model, sys.argv[1:])
