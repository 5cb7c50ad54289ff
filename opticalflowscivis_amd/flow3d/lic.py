"""Line integral convolution with the Flow-3D model: `python -m opticalflowscivis_amd.flow3d.lic --flows flows.npy --out
lic.npy` averages a noise texture along the streamlines of the step flows on the device; `flow3d.render --field lic.npy`
turns the volumes into pictures; see opticalflowscivis_amd/lic.py."""
from ..lic import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model, 3)
