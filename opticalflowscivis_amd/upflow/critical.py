"""Critical points with UPFlow: `python -m opticalflowscivis_amd.upflow.critical --dataset rectangle2d --png-dir shots
--json report.json` finds where flow_f_out (forward in time) or flow_b_out (backward) vanishes and names each zero on the
device; `--model` is a weights file or a directory holding upflow.pkl; see opticalflowscivis_amd/critical.py."""
import sys

from ..critical import main_upflow
from .test import Test_model

if __name__ == "__main__":
    main_upflow(Test_model, sys.argv[1:])
