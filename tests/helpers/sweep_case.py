"""Stations and IDW settings of the MOS/IDW sweep evaluator fixture (tests/golden/make_sweep_golden.py) on the 7 x 9
regional grid of multires_case.py, shared by the generator and tests/test_idw_sweep_eval.py."""
import numpy as np

# nine stations on eight neighbouring nodes of the 5.5 x 8 deg grid (the first two share the node 25 N, 74 E): the
# four stations of multires_case.py are too far apart for any radius the sweep would try
EV_STATIONS = [
    {"lat": 25.3, "lon": 74.5, "elev": 287, "name": "a"}, {"lat": 24.6, "lon": 73.2, "elev": 257, "name": "b"},
    {"lat": 25.4, "lon": 81.0, "elev": 207, "name": "c"}, {"lat": 30.0, "lon": 83.1, "elev": 93, "name": "d"},
    {"lat": 31.2, "lon": 89.2, "elev": 180, "name": "e"}, {"lat": 36.4, "lon": 90.9, "elev": 181, "name": "f"},
    {"lat": 35.5, "lon": 98.9, "elev": 164, "name": "g"}, {"lat": 30.9, "lon": 97.0, "elev": 290, "name": "h"},
    {"lat": 41.0, "lon": 105.0, "elev": 235, "name": "i"}]
# the scripts' powers with radii scaled to the ~600 x 800 km cells
EV_CONFIGS = [
    (2.0, 2400.0, "p2.0_r2400"), (2.0, 1600.0, "p2.0_r1600"), (2.0, 1200.0, "p2.0_r1200"), (2.0, 900.0, "p2.0_r900"),
    (2.0, 700.0, "p2.0_r700"), (3.0, 2400.0, "p3.0_r2400"), (3.0, 1200.0, "p3.0_r1200"), (3.0, 900.0, "p3.0_r900"),
    (1.5, 2400.0, "p1.5_r2400"), (1.5, 1200.0, "p1.5_r1200")]


def lapse_elev():
    """np.float64, as the scripts' MEAN_STATION_ELEV reaches apply_lapse through argparse's default."""
    return np.mean([s["elev"] for s in EV_STATIONS])
