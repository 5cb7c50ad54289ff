"""FTLE fields with the Flow-2D model: `python -m opticalflowscivis_amd.flow2d.ftle --flows flows.npy --window 3 --out
ftle.npy` advects a lattice through the step flows (the model's, or given ones) and reduces the flow map to Lyapunov
exponents; see opticalflowscivis_amd/ftle.py."""
from ..ftle import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model, 2)
