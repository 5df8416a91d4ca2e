"""The device forms of the Python state classes against the rules of
wrapper_cases.py, at the same tiny shapes (3 tables or connections, one
5,000-byte value): growth by cap_for with the log's prefix kept, an empty table
list that stays a list, and every collapsed host/device pair (read_encoder,
read_decoder, release_blocked, keys) giving the host form's result on the same
inputs.  Each case is a handful of launches."""
import pytest

import ack_cases as ac
import wrapper_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev(codec):
    return ac.Dev(codec, 0)


@pytest.mark.parametrize("case", wc.GROWTH, ids=lambda f: f.__name__)
def test_growth(dev, case):
    case(dev)


@pytest.mark.parametrize("case", wc.EMPTY, ids=lambda f: f.__name__)
def test_empty_list_is_a_list(dev, case):
    case(dev)
