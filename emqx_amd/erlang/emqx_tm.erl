%% emqx_tm -- Erlang face of the MI355X topic-matching engine (NIF: emqx_tm_nif.c).
%%
%% Drop-in for the read side of emqx_trie (src/emqx_trie.erl) used by
%% emqx_router:match_routes/1 (src/emqx_router.erl:127-141), plus the trie
%% mutations the router applies after its mnesia transaction commits.
%% See INTEGRATION.md for the two-line change in emqx_router.
-module(emqx_tm).

-export([ new/1
        , insert/2
        , delete/2
        , lookup/2
        , empty/1
        , match/2
        , match_async/3
        , match_batch/2
        , topic_match/2
        , route_add/3
        , route_delete/3
        , route_apply/2
        , subscribe/4
        , subscribe/5
        , get_subopts/3
        , unsubscribe/4
        , subscriber_down/3
        , dispatch_batch/2
        , deliver_batch/2
        , deliver_batch/3
        , session_deliver_batch/3
        , session_window_batch/4
        , match_routes_batch/2
        , rules_match/4
        , acl_new/2
        , acl_load/2
        , acl_check/4
        , check_acl/4
        , shared_subscribe/4
        , shared_subscribe/5
        , shared_flag/2
        , shared_unsubscribe/4
        , shared_member_down/2
        , shared_dispatch_batch/4
        , shared_dispatch/3
        ]).

-on_load(init/0).

init() ->
    Dir = case code:priv_dir(emqx) of
              {error, _} -> "priv";
              D -> D
          end,
    erlang:load_nif(filename:join(Dir, "emqx_tm_nif"), 0).

%% new(Device) binds one GPU; new([Device]) one engine over several GPUs (one
%% host trie, an HBM replica on each, per-publish matches dealt over them and
%% batch calls spread over them).  The async pipelines start here.
-spec(new(non_neg_integer() | [non_neg_integer()]) -> {ok, reference()} | {error, term()}).
new(_Devices) -> erlang:nif_error(nif_not_loaded).

%% emqx_trie:insert/1
-spec(insert(reference(), binary()) -> ok | {error, term()}).
insert(_Engine, _Topic) -> erlang:nif_error(nif_not_loaded).

%% emqx_trie:delete/1
-spec(delete(reference(), binary()) -> ok | {error, term()}).
delete(_Engine, _Topic) -> erlang:nif_error(nif_not_loaded).

%% emqx_trie:lookup/1 -> [#trie_node{}]
-spec(lookup(reference(), binary() | root) -> list()).
lookup(_Engine, _NodeId) -> erlang:nif_error(nif_not_loaded).

%% emqx_trie:empty/0
-spec(empty(reference()) -> boolean()).
empty(_Engine) -> erlang:nif_error(nif_not_loaded).

%% emqx_trie:match/1 (sorted, deduplicated).  The calling process queues its
%% topic and waits for its own reply: every publishing process can have a
%% match in flight, and the engine batches whatever is queued onto the device.
-spec(match(reference(), binary()) -> [binary()] | {error, term()}).
match(Engine, Topic) ->
    Ref = make_ref(),
    case match_async(Engine, Topic, Ref) of
        ok -> receive {emqx_tm_match, Ref, Result} -> Result end;
        {error, _} = Error -> Error
    end.

%% Queue one match; the reply {emqx_tm_match, Ref, [Filter] | {error, Reason}}
%% arrives as a message (runs on a normal scheduler: it only enqueues).
-spec(match_async(reference(), binary(), reference()) -> ok | {error, term()}).
match_async(_Engine, _Topic, _Ref) -> erlang:nif_error(nif_not_loaded).

%% match/1 over a batch of publishes, one device pipeline
-spec(match_batch(reference(), [binary()]) -> [[binary()]]).
match_batch(_Engine, _Topics) -> erlang:nif_error(nif_not_loaded).

%% emqx_topic:match/2 on binaries
-spec(topic_match(binary(), binary()) -> boolean()).
topic_match(_Name, _Filter) -> erlang:nif_error(nif_not_loaded).

%% emqx_router:do_add_route/2 after the mnesia transaction committed.
%% DestId: the caller's id of the route's aggre/1 destination (node(), or the
%% share Group of a {Group, Node} dest), src/emqx_broker.erl:250-261.
-spec(route_add(reference(), binary(), non_neg_integer()) -> ok | {error, term()}).
route_add(_Engine, _Topic, _DestId) -> erlang:nif_error(nif_not_loaded).

%% emqx_router:do_delete_route/2 after the commit.
-spec(route_delete(reference(), binary(), non_neg_integer()) -> ok | {error, term()}).
route_delete(_Engine, _Topic, _DestId) -> erlang:nif_error(nif_not_loaded).

%% Cluster route delta feed: emqx_route table events in order, one call
%% (mnesia replication of remote routes, cleanup_routes/1 on nodedown,
%% shared-subscription {Group, node()} routes).  Absent delete_object = no-op.
-spec(route_apply(reference(), [{write | delete_object, binary(), non_neg_integer()}])
      -> {ok, non_neg_integer()} | {error, term()}).
route_apply(_Engine, _Events) -> erlang:nif_error(nif_not_loaded).

%% Local subscriber bag (emqx_broker do_subscribe/4, do_unsubscribe/4,
%% subscriber_down/1, non-shared): SubId = the caller's id of the subscriber
%% pid, NodeDestId = its id of node() in route_add/3.
-spec(subscribe(reference(), binary(), non_neg_integer(), non_neg_integer()) -> ok | {error, term()}).
subscribe(_Engine, _Topic, _SubId, _NodeDestId) -> erlang:nif_error(nif_not_loaded).

%% subscribe/3 with the ?SUBOPTION entry (src/emqx_broker.erl:127-136):
%% SubOpts = {QoS, NL, RAP, RH, SubIdent} (SubIdent 0 = none).  A new
%% subscription stores them; an existing one merges them (the four flags are
%% replaced, SubIdent only when non-zero).  subscribe/4 is the defaults.
-type(subopts() :: {0..2, 0..1, 0..1, 0..2, non_neg_integer()}).
-spec(subscribe(reference(), binary(), non_neg_integer(), non_neg_integer(), subopts()) -> ok | {error, term()}).
subscribe(_Engine, _Topic, _SubId, _NodeDestId, _SubOpts) -> erlang:nif_error(nif_not_loaded).

%% emqx_broker:get_subopts/2 (:373-386).
-spec(get_subopts(reference(), binary(), non_neg_integer()) -> {ok, subopts()} | undefined | {error, term()}).
get_subopts(_Engine, _Topic, _SubId) -> erlang:nif_error(nif_not_loaded).

-spec(unsubscribe(reference(), binary(), non_neg_integer(), non_neg_integer()) -> ok | {error, term()}).
unsubscribe(_Engine, _Topic, _SubId, _NodeDestId) -> erlang:nif_error(nif_not_loaded).

-spec(subscriber_down(reference(), non_neg_integer(), non_neg_integer()) -> {ok, non_neg_integer()} | {error, term()}).
subscriber_down(_Engine, _SubId, _NodeDestId) -> erlang:nif_error(nif_not_loaded).

%% emqx_broker:dispatch/2 fan-out for a batch of publishes: per publish the
%% SubIds to deliver to ([] = {error, no_subscribers}).
-spec(dispatch_batch(reference(), [binary()]) -> [[non_neg_integer()]]).
dispatch_batch(_Engine, _Topics) -> erlang:nif_error(nif_not_loaded).

%% The same deliveries grouped by subscriber on the device: SubIds ascending,
%% each with its {PublishIndex0, To} in mailbox order (src/emqx_broker.erl:
%% 298-302), so the caller sends one inbox per SubPid, in order, and
%% emqx_misc:drain_deliver/1 collects it whole (INTEGRATION.md).
-spec(deliver_batch(reference(), [binary()])
      -> [{non_neg_integer(), [{non_neg_integer(), binary()}]}] | {error, term()}).
deliver_batch(_Engine, _Topics) -> erlang:nif_error(nif_not_loaded).

%% deliver_batch/2 with the shared deliveries in the inboxes (emqx_shared_sub:
%% do_dispatch/4 ends in the same SubPid ! {deliver, Topic, Msg},
%% src/emqx_shared_sub.erl:135-158, shared_dispatch_ack_enabled = false).
%% Flags = [] | [shared_flag()]: with a strategy flag every {To, Group} route of
%% a publish delivers to one picked member, behind the ordinary subscribers of
%% To (src/emqx_broker.erl:255-261), as {PublishIndex0, {To, GroupDestId}}.
-type(shared_flag() :: shared_round_robin | {shared_random, non_neg_integer()} | {shared_hash, [non_neg_integer()]}).
-spec(deliver_batch(reference(), [binary()], [shared_flag()])
      -> [{non_neg_integer(), [{non_neg_integer(), binary() | {binary(), non_neg_integer()}}]}] | {error, term()}).
deliver_batch(_Engine, _Topics, _Flags) -> erlang:nif_error(nif_not_loaded).

%% The strategy flag of deliver_batch/3, session_deliver_batch/3 and
%% session_window_batch/4 for a batch published by Froms (#message.from of
%% every publish, in order): the hash keys are erlang:phash2(From), the
%% reference's own (src/emqx_shared_sub.erl:267-268), as in shared_dispatch/3;
%% random is seeded from the caller's rand state.
-spec(shared_flag(random | round_robin | hash, [term()]) -> shared_flag()).
shared_flag(hash, Froms) -> {shared_hash, [erlang:phash2(From) || From <- Froms]};
shared_flag(random, _Froms) -> {shared_random, rand:uniform(16#100000000) - 1};
shared_flag(round_robin, _Froms) -> shared_round_robin.

%% deliver_batch/2 after emqx_channel:ignore_local/3 (src/emqx_channel.erl:682-693)
%% and emqx_session:enrich_subopts/3 (src/emqx_session.erl:500-529), on the
%% device: what each session sends.  A publish is {FromSubId | none, QoS,
%% Retain, Retained, Topic}; a delivery is {{PublishIndex0, Filter}, QoS,
%% Retain, NL, SubIdent} (SubIdent 0 = none), the inboxes that lost every
%% delivery left out.  Flags: upgrade_qos (#session.upgrade_qos = true for the
%% whole call), nl_all (drop every own delivery, not only the leading run), and
%% at most one shared_flag(): the shared deliveries are then in the inboxes
%% (deliver_batch/3), their pair {PublishIndex0, {Filter, GroupDestId}}; the
%% options are those of {SubId, Filter} (shared_subscribe/5), and a member
%% without any gets the publish as it is.
-type(publish() :: {non_neg_integer() | none, 0..2, boolean(), boolean(), binary()}).
-type(delivery() :: {{non_neg_integer(), binary() | {binary(), non_neg_integer()}}, 0..2, boolean(), boolean(),
                     non_neg_integer()}).
-spec(session_deliver_batch(reference(), [publish()], [upgrade_qos | nl_all | shared_flag()])
      -> [{non_neg_integer(), [delivery()]}] | {error, term()}).
session_deliver_batch(_Engine, _Publishes, _Flags) -> erlang:nif_error(nif_not_loaded).

%% session_deliver_batch/3, then what emqx_channel:handle_deliver/2
%% (src/emqx_channel.erl:657-680) decides for every delivery, on the device
%% (tm_batch_window): emqx_session:deliver/2 (src/emqx_session.erl:421-457) for
%% a connected session -- packet ids from NextPktId, the inflight window, the
%% mqueue once it is full -- and enqueue/2 (:459-472) for a disconnected one.
%% Sessions = {Default, [Session]}, the list ascending by SubId; Default (its
%% SubId ignored) stands for a subscriber not listed.  host = a session with a
%% priority table: left to the caller, every delivery comes back as host.
%% Per subscriber: {SubId, {NextPktId, NDroppedOld, NQueued}, Sends}; the
%% caller pops NDroppedOld messages off the front of the queue it holds and
%% appends the deliveries marked queued, in order.
-type(session() :: {non_neg_integer(), 1..65535, [disconnected | store_qos0 | host],
                    non_neg_integer() | unbounded, non_neg_integer(), non_neg_integer()}).
-type(disp() :: send0 | send | queued | dropped_qos0 | dropped_queue_full | host).
-spec(session_window_batch(reference(), [publish()], {session(), [session()]}, [upgrade_qos | nl_all | shared_flag()])
      -> [{non_neg_integer(), {1..65535, non_neg_integer(), non_neg_integer()},
           [{disp(), 1..65535 | undefined, delivery()}]}] | {error, term()}).
session_window_batch(_Engine, _Publishes, _Sessions, _Flags) -> erlang:nif_error(nif_not_loaded).

%% Shared-subscription members (emqx_shared_sub's handle_call({subscribe |
%% unsubscribe, Group, Topic, SubPid}) and cleanup_down/1,
%% src/emqx_shared_sub.erl:297-315, 358-367): GroupDestId = the caller's id of
%% {Group, _} in route_add/3; the first member of (Group, Topic) adds that
%% route, the last one deletes it.
-spec(shared_subscribe(reference(), binary(), non_neg_integer(), non_neg_integer()) -> ok | {error, term()}).
shared_subscribe(_Engine, _Topic, _GroupDestId, _SubId) -> erlang:nif_error(nif_not_loaded).

%% emqx_broker:subscribe/3 with share => Group (src/emqx_broker.erl:127-136,
%% 145-163) in front of shared_subscribe/4: SubOpts go under {SubId, Topic}, the
%% key of a non-shared subscription's too; a key that has options already only
%% merges them and joins no group (the `Existed` branch, :129-135).
%% shared_unsubscribe/4 and shared_member_down/2 delete what this call stored.
-spec(shared_subscribe(reference(), binary(), non_neg_integer(), non_neg_integer(), subopts()) -> ok | {error, term()}).
shared_subscribe(_Engine, _Topic, _GroupDestId, _SubId, _SubOpts) -> erlang:nif_error(nif_not_loaded).

-spec(shared_unsubscribe(reference(), binary(), non_neg_integer(), non_neg_integer()) -> ok | {error, term()}).
shared_unsubscribe(_Engine, _Topic, _GroupDestId, _SubId) -> erlang:nif_error(nif_not_loaded).

-spec(shared_member_down(reference(), non_neg_integer()) -> {ok, non_neg_integer()} | {error, term()}).
shared_member_down(_Engine, _SubId) -> erlang:nif_error(nif_not_loaded).

%% emqx_shared_sub:dispatch/3 for every {To, Group} route of every publish: per
%% publish [{To, GroupDestId, SubId}].  hash: Arg = [erlang:phash2(ClientId)],
%% one per publish; random: Arg = the seed; round_robin: Arg is ignored.
-spec(shared_dispatch_batch(reference(), [binary()], random | round_robin | hash, [non_neg_integer()] | non_neg_integer())
      -> [[{binary(), non_neg_integer(), non_neg_integer()}]] | {error, term()}).
shared_dispatch_batch(_Engine, _Topics, _Strategy, _Arg) -> erlang:nif_error(nif_not_loaded).

%% The same for a batch of {From, Topic} publishes (From = #message.from, the
%% publisher's client id, src/emqx_shared_sub.erl:113-115) under Strategy: the
%% hash keys are erlang:phash2(From), the reference's own (:267-268); random is
%% seeded from the caller's rand state.
-spec(shared_dispatch(reference(), [{term(), binary()}], random | round_robin | hash)
      -> [[{binary(), non_neg_integer(), non_neg_integer()}]] | {error, term()}).
shared_dispatch(Engine, Publishes, hash) ->
    {Froms, Topics} = lists:unzip(Publishes),
    shared_dispatch_batch(Engine, Topics, hash, [erlang:phash2(From) || From <- Froms]);
shared_dispatch(Engine, Publishes, random) ->
    shared_dispatch_batch(Engine, [T || {_, T} <- Publishes], random, rand:uniform(16#100000000) - 1);
shared_dispatch(Engine, Publishes, round_robin) ->
    shared_dispatch_batch(Engine, [T || {_, T} <- Publishes], round_robin, 0).

%% aggre(match_routes(Topic)) for a batch of publishes, resolved on the device.
-spec(match_routes_batch(reference(), [binary()]) -> [[{binary(), non_neg_integer()}]]).
match_routes_batch(_Engine, _Topics) -> erlang:nif_error(nif_not_loaded).

%% emqx_topic:match/2 of every name against every rule (ACL: DollarRule = false,
%% rewrite / tracer filters: true); per name the indices of the matching rules.
-spec(rules_match(reference(), [binary()], [binary()], boolean()) -> [[non_neg_integer()]]).
rules_match(_Engine, _Names, _Rules, _DollarRule) -> erlang:nif_error(nif_not_loaded).

%% A compiled, immutable ACL rule set on the engine's devices.  Rules in the
%% NIF's form: {A, all} | {A, Who, Access, [Topic | {eq, Topic}]} with binary
%% topics and Who as emqx_access_rule:compile/1 leaves it (ipaddr as
%% {ipaddr, {Start, End, Len}}); acl_load/2 makes them from acl.conf terms.
-spec(acl_new(reference(), list()) -> {ok, reference()} | {error, term()}).
acl_new(_Engine, _Rules) -> erlang:nif_error(nif_not_loaded).

%% The terms of etc/acl.conf (file:consult/1) -> a rule set, in the file's
%% order: emqx_mod_acl_internal:rules_from_file/1 (src/emqx_mod_acl_internal.erl:
%% 92-98) with the publish/subscribe split left to the device's access mask.
-spec(acl_load(reference(), [emqx_access_rule:rule()]) -> {ok, reference()} | {error, term()}).
acl_load(Engine, Terms) ->
    acl_new(Engine, [acl_rule(emqx_access_rule:compile(Term)) || Term <- Terms]).

acl_rule({A, all}) -> {A, all};
acl_rule({A, Who, Access, Topics}) -> {A, Who, Access, [acl_topic(T) || T <- Topics]}.

%% compiled topics are word lists: the device takes their bytes
acl_topic({eq, Words}) -> {eq, emqx_topic:join(Words)};
acl_topic({pattern, Words}) -> emqx_topic:join(Words);
acl_topic(Words) -> emqx_topic:join(Words).

%% emqx_mod_acl_internal:check_acl/5 for a batch: Clients =
%% [{ClientId | undefined, Username | undefined, PeerHost | undefined}],
%% Requests = [{ClientIndex (0-based), publish | subscribe, Topic}] ->
%% [{allow | deny | nomatch, RuleIndex | none}].
-spec(acl_check(reference(), reference(), list(), list()) -> list() | {error, term()}).
acl_check(_Engine, _Acl, _Clients, _Requests) -> erlang:nif_error(nif_not_loaded).

%% emqx_access_control:check_acl/3 (src/emqx_access_control.erl:47-67, no ACL
%% cache) for a batch of {ClientInfo, PubSub, Topic}: nomatch falls to the
%% zone's acl_nomatch, anything but allow denies.  Any other PubSub sees no
%% rule (emqx_mod_acl_internal:lookup/2).
-spec(check_acl(reference(), reference(), [{map(), atom(), binary()}], allow | deny) -> [allow | deny]).
check_acl(Engine, Acl, Requests, AclNomatch) ->
    Default = case AclNomatch of allow -> allow; _ -> deny end,
    Known = [R || R = {_, PubSub, _} <- Requests, PubSub =:= publish orelse PubSub =:= subscribe],
    Clients = [{maps:get(clientid, CI, undefined), maps:get(username, CI, undefined),
                maps:get(peerhost, CI, undefined)} || {CI, _, _} <- Known],
    Reqs = [{I, PubSub, Topic} || {I, {_, PubSub, Topic}} <- lists:zip(lists:seq(0, length(Known) - 1), Known)],
    case acl_check(Engine, Acl, Clients, Reqs) of
        {error, _} = Error -> Error;
        Results -> acl_fold(Requests, Results, Default)
    end.

acl_fold([], [], _Default) -> [];
acl_fold([{_, PubSub, _} | Reqs], [{Verdict, _Rule} | Results], Default)
  when PubSub =:= publish; PubSub =:= subscribe ->
    [case Verdict of nomatch -> Default; allow -> allow; deny -> deny end | acl_fold(Reqs, Results, Default)];
acl_fold([_ | Reqs], Results, Default) ->
    [Default | acl_fold(Reqs, Results, Default)].
