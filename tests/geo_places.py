"""The places the geography tests build their worlds at.

Every other test of the suite uses the generator's default centre, 47N 8E: positive coordinates,
cos(lat) = 0.68, longitudes where one float32 step is 1e-6 degrees.  These centres add negative
and near-zero coordinates, both ends of the longitude range (one float32 step of 1.5e-5 degrees,
1.6 m at the equator), the equator and 78N (a degree of longitude a fifth of a degree of latitude).

A world that spans the +-180 degree line is out of scope: the graph's grid is linear in longitude
(DESIGN.md §8), so the two centres at 179.95 stay on their side of it (a 24 x 24 world at 100 m is
0.04 degrees wide there at most).
"""
from reporter_amd import world

HOME = "zurich"
PLACES = {
    "zurich": (47.0, 8.0),            # the generator's default
    "san_francisco": (37.77, -122.42),
    "sydney": (-33.87, 151.21),
    "ushuaia": (-54.8, -68.3),
    "tromso": (69.65, 18.96),
    "null_island": (0.0, 0.0),
    "fiji": (-16.8, 179.95),
    "alaska": (51.9, -179.95),
    "svalbard": (78.22, 15.65),
    "quito": (0.0, -78.5),
}
NAMES = tuple(PLACES)


def place_kw(name):
    lat, lon = PLACES[name]
    return dict(center_lat=lat, center_lon=lon)


def build_place_world(name, directory, rows=24, cols=24, block_m=100.0, seed=5, cell_m=None):
    """A synthetic grid world centred on the place, written into ``directory``; returns its path."""
    path = "%s/%s_%dx%d.rmg" % (directory, name, rows, cols)
    return world.build_world(path, rows, cols, block_m, seed=seed, cell_m=cell_m, **place_kw(name))


def build_place_city(name, directory, rows=24, cols=24, seed=7):
    """The irregular OSM city (world.build_city) centred on the place."""
    return world.build_city("%s/%s_city.rmg" % (directory, name), rows=rows, cols=cols, seed=seed, **place_kw(name))


def place_traces(path, n_traces=12, n_points=120, seed=9, **kw):
    kw.setdefault("rate_s", 1.0)
    kw.setdefault("noise_m", 5.0)
    return world.generate_traces(path, n_traces=n_traces, n_points=n_points, seed=seed, **kw)
