"""
Every option of mdhip_set_option is set by at least one test. The keys are read from the strcmp(key, "...") chain of
csrc/mdhip_ctx.hip; a key counts as tested when some file under tests/ holds set_option("key", names it as a key of
an options dict ("key": ...), or quotes it while it calls set_option with a variable key (the loops over tuples of
keys: `for key, val in zip(("seg_frame", "seg_cap", ...), cfg): ctx.set_option(key, val)`). An option that only
bench.py or tools/ flip selects code that nothing checks: a new key needs a test that sets it (results never depend on
an option, so the test compares them with a reference under every value), or a line in RETIRED below with the reason.
"""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# keys the library accepts and ignores
RETIRED = {
    "rdf_relblock",  # the f32 records are relative to their whole tile's centre since the packed sweep: accepted, no effect
}

VARIABLE_KEY = re.compile(r"set_option\(\s*[A-Za-z_]\w*\s*,")  # set_option(key, ...): the key comes from a loop


def _option_keys():
    with open(os.path.join(REPO, "mdproptools_amd", "csrc", "mdhip_ctx.hip")) as fh:
        src = fh.read()
    body = src[src.index("int mdhip_set_option("):]
    body = body[:body.index("unknown key")]
    return re.findall(r'strcmp\(key, "([a-z0-9_]+)"\)', body)


def _test_sources():
    out = {}
    for root, _dirs, files in os.walk(os.path.join(REPO, "tests")):
        for name in files:
            if name.endswith(".py") and os.path.join(root, name) != os.path.abspath(__file__):
                with open(os.path.join(root, name), errors="replace") as fh:
                    out[os.path.relpath(os.path.join(root, name), REPO)] = fh.read()
    return out


def test_every_option_is_set_by_a_test():
    keys = _option_keys()
    assert len(keys) > 40 and len(set(keys)) == len(keys), keys  # (the chain was found, and names no key twice)
    assert RETIRED <= set(keys), sorted(RETIRED - set(keys))  # (a retired key that is gone leaves this list too)
    sources = _test_sources()
    untested = []
    for key in keys:
        if key in RETIRED:
            continue
        uses = re.compile(r'set_option\(\s*["\']%s["\']|["\']%s["\']\s*:' % (key, key))
        quoted = re.compile(r'["\']%s["\']' % key)
        if not any(uses.search(text) or (VARIABLE_KEY.search(text) and quoted.search(text)) for text in sources.values()):
            untested.append(key)
    assert not untested, "options no test sets: %s" % ", ".join(untested)
