"""Pathlines with UPFlow: `python -m opticalflowscivis_amd.upflow.trace --dataset rectangle2d --direction bwd
--seed-grid 8 --json report.json` follows seeded particles through flow_f_out (forward in time) or flow_b_out
(backward); `--model` is a weights file or a directory holding upflow.pkl; see opticalflowscivis_amd/trace.py."""
import sys

from ..trace import main_upflow
from .test import Test_model

if __name__ == "__main__":
    main_upflow(Test_model, sys.argv[1:])
