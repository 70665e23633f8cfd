"""What the three kinds of schedule (wrench, vehicle, wind) say when they refuse tables or ids: every message, whole, as a literal.
The public checks of ``raptor_amd.disturbances``, ``raptor_amd.vehicles`` and ``raptor_amd.winds`` share one implementation
(``raptor_amd.schedules``); the wording is each kind's own and must not drift.  No library, no GPU."""
import numpy as np
import pytest

from raptor_amd import disturbances, vehicles, winds

# kind -> (check_tables, check_*_ids, columns, a valid entry)
KINDS = {"wrench": (disturbances.check_tables, disturbances.check_wrench_ids, 6, 0.0),
         "vehicle": (vehicles.check_tables, vehicles.check_vehicle_ids, 4, 1.0),
         "wind": (winds.check_tables, winds.check_wind_ids, 4, 0.5)}

MESSAGES = {
    "wrench": {
        "dtype": "a wrench bank is a float32 NumPy array [M, rows, 6] or a list of M [rows, 6] tables",
        "dtype_in_list": "a wrench table is a float32 NumPy array [rows, 6] (raptor_amd.disturbances builds them)",
        "rank": "a wrench bank has shape [M >= 1, rows >= 1, 6]; got (8, 6)",
        "rank_in_list": "a wrench table has shape [rows >= 1, 6]: force, torque; got (6,)",
        "columns": "a wrench bank has shape [M >= 1, rows >= 1, 6]; got (3, 8, 7)",
        "not_an_array": "a wrench bank is a float32 NumPy array [M, rows, 6] or a list of M [rows, 6] tables",
        "empty_list": "a wrench bank holds at least one table",
        "unequal": "the tables of a wrench bank have the same number of rows; got 8, 5",
        "nan_t1_r4": "a wrench table holds finite entries only",
        "inf_t1_r4_in_list": "a wrench table holds finite entries only",
        "ids_length": "wrench ids must hold one id per env: 5 ids for 4 envs",
        "ids_rank": "wrench ids must hold one id per env: (2, 2) ids for 4 envs",
        "ids_float": "wrench ids must be integers",
        "ids_bool": "wrench ids must be integers",
        "ids_out_of_range": "wrench id out of range: env 2 names table 3 of a bank of 3",
        "ids_negative": "wrench id out of range: env 3 names table -1 of a bank of 3",
    },
    "vehicle": {
        "dtype": "a vehicle bank is a float32 NumPy array [M, rows, 4] or a list of M [rows, 4] tables",
        "dtype_in_list": "a vehicle table is a float32 NumPy array [rows, 4] (raptor_amd.vehicles builds them)",
        "rank": "a vehicle bank has shape [M >= 1, rows >= 1, 4]; got (8, 4)",
        "rank_in_list": "a vehicle table has shape [rows >= 1, 4]: mass, inertia, thrust, motor_tau; got (4,)",
        "columns": "a vehicle bank has shape [M >= 1, rows >= 1, 4]; got (3, 8, 5)",
        "not_an_array": "a vehicle bank is a float32 NumPy array [M, rows, 4] or a list of M [rows, 4] tables",
        "empty_list": "a vehicle bank holds at least one table",
        "unequal": "the tables of a vehicle bank have the same number of rows; got 8, 5",
        "nan_t1_r4": "a vehicle table holds positive finite factors only: table 1, row 4, column 2 (thrust)",
        "inf_t1_r4_in_list": "a vehicle table holds positive finite factors only: table 1, row 4, column 1 (inertia)",
        "zero_factor": "a vehicle table holds positive finite factors only: table 1, row 4, column 2 (thrust)",
        "negative_factor_in_list": "a vehicle table holds positive finite factors only: table 1, row 4, column 0 (mass)",
        "ids_length": "vehicle ids must hold one id per env: 5 ids for 4 envs",
        "ids_rank": "vehicle ids must hold one id per env: (2, 2) ids for 4 envs",
        "ids_float": "vehicle ids must be integers",
        "ids_bool": "vehicle ids must be integers",
        "ids_out_of_range": "vehicle id out of range: env 2 names table 3 of a bank of 3",
        "ids_negative": "vehicle id out of range: env 3 names table -1 of a bank of 3",
    },
    "wind": {
        "dtype": "a wind bank is a float32 NumPy array [M, rows, 4] or a list of M [rows, 4] tables",
        "dtype_in_list": "a wind table is a float32 NumPy array [rows, 4] (raptor_amd.winds builds them)",
        "rank": "a wind bank has shape [M >= 1, rows >= 1, 4]; got (8, 4)",
        "rank_in_list": "a wind table has shape [rows >= 1, 4]: wx, wy, wz, drag; got (4,)",
        "columns": "a wind bank has shape [M >= 1, rows >= 1, 4]; got (3, 8, 5)",
        "not_an_array": "a wind bank is a float32 NumPy array [M, rows, 4] or a list of M [rows, 4] tables",
        "empty_list": "a wind bank holds at least one table",
        "unequal": "the tables of a wind bank have the same number of rows; got 8, 5",
        "nan_t1_r4": "a wind table holds a non-finite entry: table 1, row 4, column 2 (wz)",
        "inf_t1_r4_in_list": "a wind table holds a non-finite entry: table 1, row 4, column 1 (wy)",
        "negative_drag": "a wind table holds a negative drag: table 1, row 4, column 3 (drag)",
        "negative_drag_in_list": "a wind table holds a negative drag: table 1, row 4, column 3 (drag)",
        "ids_length": "wind ids must hold one id per env: 5 ids for 4 envs",
        "ids_rank": "wind ids must hold one id per env: (2, 2) ids for 4 envs",
        "ids_float": "wind ids must be integers",
        "ids_bool": "wind ids must be integers",
        "ids_out_of_range": "wind id out of range: env 2 names table 3 of a bank of 3",
        "ids_negative": "wind id out of range: env 3 names table -1 of a bank of 3",
    },
}


def _bad_inputs(kind):
    """name -> (check, arguments): the fixed list of bad inputs of one kind; 3 tables of 8 rows, 4 envs"""
    check_tables, check_ids, cols, fill = KINDS[kind]
    good = np.full((3, 8, cols), fill, np.float32)

    def with_entry(t, r, c, value, as_list=False):
        a = good.copy()
        a[t, r, c] = value
        return list(a) if as_list else a

    tables = {
        "dtype": good.astype(np.float64),
        "dtype_in_list": [good[0], good[1].astype(np.float64)],
        "rank": good[0],
        "rank_in_list": [good[0], good[1][0]],
        "columns": np.full((3, 8, cols + 1), fill, np.float32),
        "not_an_array": "tables",
        "empty_list": [],
        "unequal": [good[0], good[1][:5]],
        "nan_t1_r4": with_entry(1, 4, 2, np.nan),
        "inf_t1_r4_in_list": with_entry(1, 4, 1, np.inf, as_list=True),
    }
    if kind == "vehicle":
        tables["zero_factor"] = with_entry(1, 4, 2, 0.0)
        tables["negative_factor_in_list"] = with_entry(1, 4, 0, -1.0, as_list=True)
    if kind == "wind":
        tables["negative_drag"] = with_entry(1, 4, 3, -0.25)
        tables["negative_drag_in_list"] = with_entry(1, 4, 3, -1.0, as_list=True)
    ids = {
        "ids_length": np.zeros(5, np.int64),
        "ids_rank": np.zeros((2, 2), np.int64),
        "ids_float": np.zeros(4, np.float32),
        "ids_bool": np.zeros(4, bool),
        "ids_out_of_range": np.array([0, 2, 3, 1]),
        "ids_negative": np.array([0, 1, 2, -1]),
    }
    out = {name: (check_tables, (t,)) for name, t in tables.items()}
    out.update({name: (check_ids, (a, 3, 4)) for name, a in ids.items()})
    return out


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_refusal_of_a_kind_word_for_word(kind):
    bad = _bad_inputs(kind)
    assert set(bad) == set(MESSAGES[kind])
    for name, (check, args) in bad.items():
        with pytest.raises(ValueError) as e:
            check(*args)
        assert str(e.value) == MESSAGES[kind][name], name


@pytest.mark.parametrize("kind", list(KINDS))
def test_good_tables_and_ids_pass(kind):
    check_tables, check_ids, cols, fill = KINDS[kind]
    good = np.full((3, 8, cols), fill, np.float32)
    for tables in (good, list(good)):
        got = check_tables(tables)
        assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, good)
    ids = check_ids([2, 0, 1, 2], 3, 4)
    assert ids.dtype == np.uint32 and ids.flags.c_contiguous and ids.tolist() == [2, 0, 1, 2]
