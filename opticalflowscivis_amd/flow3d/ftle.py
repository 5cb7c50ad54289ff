"""FTLE fields with the Flow-3D model: `python -m opticalflowscivis_amd.flow3d.ftle --seq frames.npy --window 4 --every 2
--refine 2 --direction bwd --method rk4 --out ftle.npy --classes cls.npy --json report.json` advects a lattice through
the model's step flows and reduces the flow map to Lyapunov exponents; see opticalflowscivis_amd/ftle.py."""
from ..ftle import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model, 3)
