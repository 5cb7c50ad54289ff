"""Pictures of 2-D frames, fields and UPFlow's flows: `python -m opticalflowscivis_amd.upflow.render --field vg.npy --plane
1 --tf coolwarm --flows flows.npy --png-dir shots` colour-maps every step through the transfer function and writes
flow2rgb pictures of --flows; see opticalflowscivis_amd/render.py."""
from ..render import main2d

if __name__ == "__main__":
    main2d(desc="Colour-map 2-D frames or fields; flow2rgb pictures of UPFlow's flows")
