"""Math helpers with the reference's names (reference: utils/model.py)."""
import random

from . import ops
from .variables import Sym, is_sym


def get_coords_xy(x):
    """Both get_coord calls + tf.stack of pose_encoder in one fused pass (reference networks/__init__.py:68-71).
    x [B,H,W,K] -> (mu [B,K,2] as (x,y), prob_y [B,H,K], prob_x [B,W,K])."""
    if is_sym(x):
        b, h, w, k = x.shape
        return Sym(b, k, 2), Sym(b, h, k), Sym(b, w, k)
    return ops.keypoint_head(x)


def get_coord(x, other_axis, axis_size):
    """reference get_coord (utils/model.py:63-70): returns (coordinate [B,K], probability [B,axis_size,K]).
    other_axis=2 -> y (softmax over H), other_axis=1 -> x (softmax over W)."""
    mu, prob_y, prob_x = get_coords_xy(x)
    if other_axis == 2:
        assert axis_size == x.shape[1]
        return mu[:, :, 1], prob_y
    assert other_axis == 1 and axis_size == x.shape[2]
    return mu[:, :, 0], prob_x


def get_gaussian_maps(mu, shape_hw, inv_std=14.3):
    """reference get_gaussian_maps (utils/model.py:49-60): mu [B,K,2] (x,y) -> [B,H,W,K]."""
    if is_sym(mu):
        return Sym(mu.shape[0], shape_hw[0], shape_hw[1], mu.shape[1])
    return ops.gaussian_maps(mu, int(shape_hw[0]), int(shape_hw[1]), inv_std)


def get_random_color(pastel_factor=0.5, rng=None):
    """reference get_random_color (utils/model.py:13-14); ``uniform(0, 1)`` is ``0 + 1 * random()``."""
    r = random if rng is None else rng
    return [(x + pastel_factor) / (1.0 + pastel_factor) for x in [r.uniform(0, 1.0) for _ in [1, 2, 3]]]


def color_distance(c1, c2):
    """reference color_distance (utils/model.py:17-18): L1 distance."""
    return sum([abs(x[0] - x[1]) for x in zip(c1, c2)])


def generate_new_color(existing_colors, pastel_factor=0.5, rng=None):
    """reference generate_new_color (utils/model.py:21-32), step for step: the first colour returns after one draw; otherwise the best of
    100 candidates by distance to the nearest existing colour, where a best distance of 0.0 counts as unset (``not max_distance``)."""
    max_distance = None
    best_color = None
    for _ in range(0, 100):
        color = get_random_color(pastel_factor=pastel_factor, rng=rng)
        if not existing_colors:
            return color
        best_distance = min([color_distance(color, c) for c in existing_colors])
        if not max_distance or best_distance > max_distance:
            max_distance = best_distance
            best_color = color
    return best_color


def get_n_colors(n, pastel_factor=0.9, rng=None):
    """reference get_n_colors (utils/model.py:35-39): ``n`` [r, g, b] lists of Python floats.  As in the reference, ``pastel_factor`` is
    ignored (0.9 is always used).  ``rng``: a ``random.Random``; None draws from the module-level ``random``, as the reference does, so
    ``get_n_colors(n, rng=random.Random(s))`` is the reference's palette after ``random.seed(s)``."""
    colors = []
    for _ in range(n):
        colors.append(generate_new_color(colors, pastel_factor=0.9, rng=rng))
    return colors


def render_point_maps(mu, shape_hw, colors, inv_std=14.3):
    """The reference's ``colorize_point_maps(get_gaussian_maps(mu, shape_hw), colors)`` (utils/model.py:42-60) in one pass, without the
    [N,H,W,K] maps: mu [N,K,2] (x,y) -> [N,H,W,3].  ``colors``: [K,3] fp32 tensor on mu's device (the palette of ``get_n_colors``, cast
    to fp32 as TF casts the float64 constant to the maps' dtype)."""
    if is_sym(mu):
        return Sym(mu.shape[0], shape_hw[0], shape_hw[1], 3)
    return ops.point_maps_rgb(mu, int(shape_hw[0]), int(shape_hw[1]), colors, inv_std)
