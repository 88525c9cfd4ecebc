"""Geometry objects of the rendering API, as plain data.

The names and call signatures are those of the reference's ``vmas/simulator/rendering.py`` (its
``Geom`` family and ``make_*`` helpers), so scenario code that builds geoms in ``extra_render`` /
``top_layer_render`` or overrides ``Entity.render`` runs unchanged.  Nothing here talks to OpenGL
or pyglet: an object only holds what it was given.  ``simulator/_render.py`` lowers a list of geoms
to the primitive table that the native rasteriser (``csrc/vmas_render.hip``) composites.

Differences from the reference: a full-angle ``make_circle`` returns a :class:`Circle` (drawn as a
true disc or ring, ``res`` is unused); ``TextLine`` objects are accepted and not drawn; ``Image``
and ``render_function_util`` are not provided.
"""
from __future__ import annotations

import math
from typing import Optional

__all__ = [
    "Geom", "Attr", "Transform", "Color", "LineWidth", "Line", "FilledPolygon", "PolyLine", "Circle", "Compound",
    "Grid", "TextLine", "make_circle", "make_ellipse", "make_polygon", "make_polyline", "make_capsule",
]


class Attr:
    pass


class Color(Attr):
    def __init__(self, vec4):
        self.vec4 = vec4


class LineWidth(Attr):
    def __init__(self, stroke):
        self.stroke = stroke


class Transform(Attr):
    def __init__(self, translation=(0.0, 0.0), rotation=0.0, scale=(1, 1)):
        self.set_translation(*translation)
        self.set_rotation(rotation)
        self.set_scale(*scale)

    def set_translation(self, newx, newy):
        self.translation = (float(newx), float(newy))

    def set_rotation(self, new):
        self.rotation = float(new)

    def set_scale(self, newx, newy):
        self.scale = (float(newx), float(newy))


class Geom:
    """Attributes apply as in the reference: the one added last is outermost."""

    def __init__(self):
        self._color = Color((0, 0, 0, 1.0))
        self.attrs = [self._color]

    def add_attr(self, attr):
        self.attrs.append(attr)

    def set_color(self, r, g, b, alpha=1):
        self._color.vec4 = (r, g, b, alpha)


class _Stroked(Geom):
    def __init__(self, width):
        super().__init__()
        self.linewidth = LineWidth(width)
        self.add_attr(self.linewidth)

    def set_linewidth(self, x):
        self.linewidth.stroke = x


class Line(_Stroked):
    def __init__(self, start=(0.0, 0.0), end=(0.0, 0.0), width: float = 1):
        super().__init__(width)
        self.start = start
        self.end = end


class PolyLine(_Stroked):
    def __init__(self, v, close):
        super().__init__(1)
        self.v = v
        self.close = close


class Grid(_Stroked):
    def __init__(self, spacing: float = 0.1, length: float = 50, width: float = 0.5):
        super().__init__(width)
        self.spacing = spacing
        self.length = length


class FilledPolygon(Geom):
    def __init__(self, v, draw_border: float = True):
        super().__init__()
        self.draw_border = draw_border
        self.v = v


class Circle(Geom):
    """A circle about the origin of its own frame: a disc when ``filled``, else a ring of GL line
    width 1 (what ``make_circle`` returns for the full angle)."""

    def __init__(self, radius: float = 10, filled: bool = True, draw_border: float = True):
        super().__init__()
        self.radius = radius
        self.filled = filled
        self.draw_border = draw_border
        self.linewidth = LineWidth(1)
        if not filled:
            self.add_attr(self.linewidth)

    def set_linewidth(self, x):
        self.linewidth.stroke = x


class Compound(Geom):
    """Its members drop their own colour and take the compound's."""

    def __init__(self, gs):
        super().__init__()
        self.gs = gs
        for g in self.gs:
            g.attrs = [a for a in g.attrs if not isinstance(a, Color)]


class TextLine(Geom):
    """Held, not drawn (text is outside the native renderer)."""

    def __init__(self, text: str = "", font_size: int = 15, x: float = 0.0, y: float = 0.0):
        super().__init__()
        self.text = text
        self.font_size = font_size
        self.x = x
        self.y = y

    def set_text(self, text, font_size: Optional[int] = None):
        self.text = text
        if font_size is not None:
            self.font_size = font_size


def make_circle(radius=10, res=30, filled=True, angle=2 * math.pi):
    if angle % (2 * math.pi) == 0:
        return Circle(radius, filled=filled)
    return make_ellipse(radius_x=radius, radius_y=radius, res=res, filled=filled, angle=angle)


def make_ellipse(radius_x=10, radius_y=5, res=30, filled=True, angle=2 * math.pi):
    points = [(math.cos(-angle / 2 + angle * i / res) * radius_x, math.sin(-angle / 2 + angle * i / res) * radius_y)
              for i in range(res)]
    if angle % (2 * math.pi) != 0:
        points.append((0, 0))
    return FilledPolygon(points) if filled else PolyLine(points, True)


def make_polygon(v, filled=True, draw_border: float = True):
    return FilledPolygon(v, draw_border=draw_border) if filled else PolyLine(v, True)


def make_polyline(v):
    return PolyLine(v, False)


def make_capsule(length, width):
    left, right, top, bottom = 0, length, width / 2, -width / 2
    box = make_polygon([(left, bottom), (left, top), (right, top), (right, bottom)])
    end0 = make_circle(width / 2)
    end1 = make_circle(width / 2)
    end1.add_attr(Transform(translation=(length, 0)))
    return Compound([box, end0, end1])
