"""Ridge surfaces (LCS) with the Flow-3D model: `python -m opticalflowscivis_amd.flow3d.ridges --seq frames.npy --window 4
--direction bwd --refine 2 --sigma 1 --strength 0.05 --fmin 0.2 --min-faces 32 --mesh-dir meshes --format ply --out
ridges.npz --json report.json` computes the FTLE fields of the model's step flows and extracts their height ridges -- the
transport barriers -- as triangle meshes on the device; `--field x.npy --plane N [--valley]` does the same for any stored
volume stack.  See opticalflowscivis_amd/ridges.py."""
from ..ridges import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model)
