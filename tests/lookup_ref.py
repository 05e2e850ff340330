"""Python big-int restatement of the lookup argument's permuted columns, the
reference of tests/test_lookup_*.py.  halo2's crates are not vendored under the
reference, so, as tests/gp_ref.py does for the grand products, the definitions
are restated here from halo2 `src/plonk/lookup/prover.rs` [3P]:

  * `compress_expressions`: fold the columns with theta,
    acc = acc * theta + column, from zero;
  * `permute_expression_pair`: sort the input's usable rows; count the table's
    usable rows in a BTreeMap; walk the sorted input: a row that is the first
    of its value copies the value into the permuted table and takes one
    instance out of the map (a value the map lacks is
    Error::ConstraintSystemFailure), every other row is remembered as
    repeated; then walk the map in key order and hand each leftover instance
    to the repeated row popped from the BACK of that list.

Values are plain integers mod r, ordered as integers (halo2's Ord on field
elements compares the canonical representation)."""


def compress(cols, theta, r):
    """out[i] = sum_k theta^(m-1-k) cols[k][i]"""
    out = [0] * len(cols[0])
    for col in cols:
        out = [(acc * theta + v) % r for acc, v in zip(out, col)]
    return out


def permute_pair(a, s, usable):
    """(A'[0 .. usable), S'[0 .. usable)), or the failing row (an int): the
    first row of the sorted input whose value the table lacks."""
    permuted_input = sorted(a[:usable])
    leftover_table_map = {}
    for coeff in s[:usable]:
        leftover_table_map[coeff] = leftover_table_map.get(coeff, 0) + 1
    permuted_table = [0] * usable
    repeated_input_rows = []
    for row, input_value in enumerate(permuted_input):
        if row == 0 or input_value != permuted_input[row - 1]:
            permuted_table[row] = input_value
            if input_value not in leftover_table_map:
                return row
            assert leftover_table_map[input_value] > 0
            leftover_table_map[input_value] -= 1
        else:
            repeated_input_rows.append(row)
    for coeff in sorted(leftover_table_map):  # BTreeMap iteration: ascending keys
        for _ in range(leftover_table_map[coeff]):
            permuted_table[repeated_input_rows.pop()] = coeff
    assert not repeated_input_rows
    return permuted_input, permuted_table
