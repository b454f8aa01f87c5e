"""No GPU: the direction-group syntax of TIGAR_PTAP_GROUPS / TIGAR_PTAP_FACTORED (kronptap.parse_direction_groups) and the
walk over the ordered table of PtAP routes (ptaproutes.first_route)."""
import types

import pytest

from tigar_amd.kronptap import parse_direction_groups
from tigar_amd.ptaproutes import first_route


def test_direction_groups_as_the_two_switches_document_them():
    assert parse_direction_groups("0;1;2", 3, True) == [[0], [1], [2]]
    assert parse_direction_groups("0,1;2", 3, True) == [[0, 1], [2]]
    assert parse_direction_groups("0,1;2", 3, False) == [[0, 1], [2]]
    # a direction the patch does not have is dropped, and so is a group left empty by that
    assert parse_direction_groups("0;1;2", 2, True) == [[0], [1]]
    assert parse_direction_groups("0,1;2", 2, False) == [[0, 1]]
    # the groups must cover every direction exactly once
    assert parse_direction_groups("0;2", 3, True) is None
    assert parse_direction_groups("0;2", 3, False) is None
    assert parse_direction_groups("0,1;1;2", 3, False) is None
    # planes refer to the last direction: TIGAR_PTAP_GROUPS wants it in the last group, TIGAR_PTAP_FACTORED does not ask
    assert parse_direction_groups("2;0,1", 3, True) is None
    assert parse_direction_groups("2;0,1", 3, False) == [[2], [0, 1]]
    assert parse_direction_groups("1,2;0", 3, True) is None
    assert parse_direction_groups("0;1,2", 3, True) == [[0], [1, 2]]


def test_route_table_is_walked_in_order_and_names_K():
    asked = []

    def route(name, applies, K):
        def run(call):
            asked.append(name)
            return K
        return name, (lambda call: applies), run

    K2, K3 = types.SimpleNamespace(), types.SimpleNamespace()
    routes = [route("absent", False, types.SimpleNamespace()), route("declines", True, None), route("second", True, K2),
              route("third", True, K3)]
    K = first_route(routes, None)
    assert K is K2 and K.ptap_route == "second"               # the first route that does not decline wins and names K
    assert asked == ["declines", "second"]                    # in order; what does not apply is not run, nor what comes after
    assert not hasattr(K3, "ptap_route")
    with pytest.raises(RuntimeError):
        first_route(routes[:2], None)
