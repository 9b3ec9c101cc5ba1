"""Reference uri_internal_test.go, ported (13 tests): address grammar,
defaults, normalisation, setters and their validation."""
import pytest

from pilosa_amd.parallel.cluster import URI

VALID = [  # uri_internal_test.go validFixture
    ("http+protobuf://index1.pilosa.com:3333", "http+protobuf", "index1.pilosa.com", 3333),
    ("index1.pilosa.com:3333", "http", "index1.pilosa.com", 3333),
    ("https://index1.pilosa.com", "https", "index1.pilosa.com", 10101),
    ("index1.pilosa.com", "http", "index1.pilosa.com", 10101),
    ("https://:3333", "https", "localhost", 3333),
    (":3333", "http", "localhost", 3333),
    ("[::1]", "http", "[::1]", 10101),
    ("[::1]:3333", "http", "[::1]", 3333),
    ("[fd42:4201:f86b:7e09:216:3eff:fefa:ed80]:3333", "http", "[fd42:4201:f86b:7e09:216:3eff:fefa:ed80]", 3333),
    ("https://[fd42:4201:f86b:7e09:216:3eff:fefa:ed80]:3333", "https", "[fd42:4201:f86b:7e09:216:3eff:fefa:ed80]", 3333),
]
INVALID = ["foo:bar", "http://foo:", "foo:", ":bar", "http://pilosa.com:129999999999999999999999993",
           "fd42:4201:f86b:7e09:216:3eff:fefa:ed80", ":65536"]


def _cmp(u, scheme, host, port):
    assert (u.scheme, u.host, u.port) == (scheme, host, port)


def test_default_uri():                          # TestDefaultURI
    _cmp(URI(), "http", "localhost", 10101)


def test_uri_with_host_port():                   # TestURIWithHostPort
    _cmp(URI.from_host_port("index1.pilosa.com", 3333), "http", "index1.pilosa.com", 3333)


def test_uri_with_invalid_host_port():           # TestURIWithInvalidHostPort
    with pytest.raises(ValueError):
        URI.from_host_port("index?.pilosa.com", 3333)


# "::" separates the parts of a pytest node id, so the two "[::1]" cases carry
# names of their own; every other case keeps the id pytest derives
_IPV6_LOOPBACK_IDS = {"[::1]": "ipv6-loopback", "[::1]:3333": "ipv6-loopback-port"}


@pytest.mark.parametrize("addr,scheme,host,port", VALID, ids=[_IPV6_LOOPBACK_IDS.get(v[0]) for v in VALID])
def test_new_uri_from_address(addr, scheme, host, port):   # TestNewURIFromAddress
    _cmp(URI.parse(addr), scheme, host, port)


@pytest.mark.parametrize("addr", INVALID)
def test_new_uri_from_address_invalid(addr):     # TestNewURIFromAddressInvalidAddress
    with pytest.raises(ValueError):
        URI.parse(addr)


def test_normalized_address():                   # TestNormalizedAddress
    assert URI.parse("http+protobuf://big-data.pilosa.com:6888").normalize() == "http://big-data.pilosa.com:6888"


def test_uri_path():                             # TestURIPath
    u = URI.parse("http+protobuf://big-data.pilosa.com:6888")
    assert u.path("/index/foo") == "http://big-data.pilosa.com:6888/index/foo"


def test_set_scheme():                           # TestSetScheme
    u = URI()
    u.set_scheme("fun")
    assert u.scheme == "fun"


def test_set_host():                             # TestSetHost
    u = URI()
    u.set_host("10.20.30.40")
    assert u.host == "10.20.30.40"


def test_set_port():                             # TestSetPort
    u = URI()
    u.set_port(9999)
    assert u.port == 9999


def test_set_invalid_scheme():                   # TestSetInvalidScheme
    with pytest.raises(ValueError):
        URI().set_scheme("?invalid")


def test_set_invalid_host():                     # TestSetInvalidHost
    with pytest.raises(ValueError):
        URI().set_host("index?.pilosa.com")


def test_host_port():                            # TestHostPort
    assert URI.from_host_port("i.pilosa.com", 15001).host_port() == "i.pilosa.com:15001"


# ---------------------------------------------------------------- pilosa_test.go TestAddressWithDefaults
# The reference lists ":", "localhost:", "127.0.0.1:" and "1.2.3.4:" as
# defaulting to port 10101, but its address grammar (uri.go addressRegexp)
# rejects a bare trailing colon and the test's error branch accepts any error
# when no error text is given: the reference answers "invalid address", and
# so does this URI.
@pytest.mark.parametrize("addr,want", [
    ("", "localhost:10101"), ("localhost", "localhost:10101"), ("127.0.0.1:10101", "127.0.0.1:10101"),
    (":10101", "localhost:10101"), (":55555", "localhost:55555"), ("1.2.3.4", "1.2.3.4:10101"),
    ("1.2.3.4:55555", "1.2.3.4:55555")])
def test_address_with_defaults(addr, want):
    u = URI() if addr == "" else URI.parse(addr)     # AddressWithDefaults: "" is the default URI
    assert u.host_port() == want


@pytest.mark.parametrize("addr", ["[invalid][addr]:port", ":", "localhost:", "127.0.0.1:", "1.2.3.4:"])
def test_address_with_defaults_invalid(addr):
    with pytest.raises(ValueError, match="invalid address"):
        URI.parse(addr)
