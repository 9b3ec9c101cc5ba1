"""Several nodes on one host with one [gossip] port: only the first can bind
it, and a UDP ping it sends to a peer "at that port" comes back to its own
socket.  The peer must not look alive because this node acknowledged its own
ping (a paused node then flipped between DOWN, reported by the others, and
READY, and every status broadcast in between hung on it)."""
import socket
import threading
import time

import pytest

from pilosa_amd.parallel.gossip_udp import UdpProber

from tests.test_swim import _udp_server, _wait


class _N:
    def __init__(self, nid):
        self.id = nid


def test_ping_req_for_a_target_at_the_helpers_own_address_is_dropped():
    a, b = _N("a"), _N("b")
    helper = UdpProber("a", "127.0.0.1", 0, lambda: [a, b], lambda n: ("127.0.0.1", helper.port))
    asker = UdpProber("c", "127.0.0.1", 0, lambda: [], lambda n: ("127.0.0.1", helper.port))
    try:
        d0 = helper.dropped
        assert not asker.ping_req(a, b, 0.2)      # b shares a's address: a's own ACK would answer
        assert helper.dropped == d0 + 1
        assert asker.ping(a, 1.0)                 # a itself still answers
    finally:
        asker.close()
        helper.close()


@pytest.mark.timeout(120)
def test_paused_peer_on_a_shared_gossip_port_is_suspected_by_the_port_holder():
    x = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    x.bind(("127.0.0.1", 0))
    gport = x.getsockname()[1]
    x.close()
    m0 = _udp_server("node0", gport, None, None)
    m1 = m2 = None
    gate = threading.Event()
    try:
        m1, m2 = _udp_server("node1", gport, None, None, m0), _udp_server("node2", gport, None, None, m0)
        assert m0.udp_prober is not None and m1.udp_prober is None and m2.udp_prober is None
        assert _wait(lambda: all(s.cluster.state == "NORMAL" and len(s.cluster.nodes) == 3 for s in (m0, m1, m2)),
                     20)
        orig = m2.handler.dispatch

        def paused(req):
            gate.wait()
            return orig(req)
        m2.handler.dispatch = paused
        assert _wait(lambda: m0.cluster.node_by_id("node2").state == "DOWN", 20)
        # the coordinator's own detector reached the verdict too, so it does not call the node alive again
        assert _wait(lambda: "node2" in m0.failure_detector.suspect_since, 10)
        flips = 0
        end = time.time() + 1.0            # ten probe intervals
        while time.time() < end:
            flips += m0.cluster.node_by_id("node2").state != "DOWN"
            time.sleep(0.02)
        assert flips == 0 and m0.cluster.node_by_id("node1").state == "READY"
        gate.set()
        m2.handler.dispatch = orig
        assert _wait(lambda: m0.cluster.node_by_id("node2").state == "READY", 20)
    finally:
        gate.set()
        for s in (m2, m1, m0):
            if s is not None:
                s.close()
