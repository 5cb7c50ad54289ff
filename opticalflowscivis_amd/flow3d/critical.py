"""Critical points with the Flow-3D model: `python -m opticalflowscivis_amd.flow3d.critical --flows flows.npy --out cp.npz
--json report.json` finds where the step flows vanish and names each zero (sink, saddle1, saddle2, source, spiral) on the
device and links the zeros of consecutive steps; see opticalflowscivis_amd/critical.py."""
from ..critical import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model, 3)
