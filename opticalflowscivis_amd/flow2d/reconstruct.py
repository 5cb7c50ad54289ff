"""Write a temporally up-sampled series with the Flow-2D model: `python -m opticalflowscivis_amd.flow2d.reconstruct
--series img.npy --exp 2 --out img_x4.npy --flows flows.npy`; see opticalflowscivis_amd/reconstruct.py."""
from ..reconstruct import main
from .model.RIFE import Model

if __name__ == "__main__":
    main(Model, 2)
