// The reference's analytic gradients, stated once for the device: what make_gradient
// (vivarium/processes/diffusion_field.py:42-206) fills a lattice with and what
// StaticField.get_concentration (vivarium/processes/static_field.py:92-119) hands an agent at
// its own position are the same arithmetic, in the same operation order.  Compiled with
// -ffp-contract=off like every unit: +, -, x, / and sqrt round as the reference's NumPy
// doubles do; exp and pow are the device library's.
#pragma once

#include <math.h>
#include <stdint.h>

#include "vk_internal.h"

// The value of `g` at (x, y), both in um.  cx, cy arrive already multiplied by the bounds.
__device__ __forceinline__ double gradient_value(const vk_gradient_spec &g, double x, double y) {
    if (g.type == VK_GRADIENT_UNIFORM) return g.p0;
    const double dx = x - g.cx, dy = y - g.cy;
    const double distance = sqrt(dx * dx + dy * dy);
    const double d = distance / 1000.0;     // um -> mm: a true division, as the reference writes it
    if (g.type == VK_GRADIENT_GAUSSIAN) return exp((-(d * d)) / (2.0 * (g.p0 * g.p0)));
    if (g.type == VK_GRADIENT_LINEAR) return g.p0 + g.p1 * d;
    return g.p1 * pow(g.p0, d);             // exponential: scale * base ** d
}

// what every entry point that takes specs checks of them on the host
static inline bool gradient_spec_ok(const vk_gradient_spec &g) {
    switch (g.type) {
    case VK_GRADIENT_UNIFORM:
    case VK_GRADIENT_LINEAR:
        return true;
    case VK_GRADIENT_GAUSSIAN:
        return g.p0 != 0.0;
    case VK_GRADIENT_EXPONENTIAL:
        return g.p0 > 0.0;
    default:
        return false;
    }
}
