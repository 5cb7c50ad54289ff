"""Line integral convolution with UPFlow: `python -m opticalflowscivis_amd.upflow.lic --dataset rectangle2d --png-dir
shots --json report.json` averages a noise texture along the streamlines of flow_f_out (forward in time) or flow_b_out
(backward) on the device; `--model` is a weights file or a directory holding upflow.pkl; see
opticalflowscivis_amd/lic.py."""
import sys

from ..lic import main_upflow
from .test import Test_model

if __name__ == "__main__":
    main_upflow(Test_model, sys.argv[1:])
