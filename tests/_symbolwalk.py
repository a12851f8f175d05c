"""Restatements of the symbol walk's device arithmetic (dd_symbol_walk.h) shared by the Meteor-M2 and Funcube host tests."""
import math


def skip(t, T, room):
    """dd_met_skip (dd_symbol_walk.h): how many plain timing += 1 samples the walk takes at once"""
    _, e = math.frexp(t)
    U2 = math.ldexp(1.0, e + 1)
    est = min(T - t, U2 - 1.0 - t)
    m = 0 if est <= 0 else int(min(math.ceil(est), room))
    while m > 0 and not (t + (m - 1) < T and t + m < U2):
        m -= 1
    while m < room and t + m < T and t + (m + 1) < U2:
        m += 1
    return m
