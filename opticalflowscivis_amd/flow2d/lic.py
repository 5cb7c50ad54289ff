"""Line integral convolution with the Flow-2D model: `python -m opticalflowscivis_amd.flow2d.lic --dataset rectangle2d
--png-dir shots --json report.json` averages a noise texture along the streamlines of the step flows (the model's, or
given ones) on the device and writes grey pictures; see opticalflowscivis_amd/lic.py."""
from ..lic import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model, 2)
