"""Write a temporally up-sampled series with the Flow-3D model: `python -m opticalflowscivis_amd.flow3d.reconstruct
--series sim.npy --exp 2 --out sim_x4.npy --flows flows.npy`; see opticalflowscivis_amd/reconstruct.py."""
from ..reconstruct import main
from .model.RIFE import Model

if __name__ == "__main__":
    main(Model, 3)
